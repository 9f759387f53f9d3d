"""Call sequences and model mutation against fresh state (tests/state_twin.py has the vocabulary: veteran, fresh twin).

Every other GPU parity test builds a model, loads its weights and makes ONE call (or N identical steps).  These tests check that a
call's result depends only on its inputs and not on what the same model, Trainer or process did before:

A. a model mutated after its first forward (frozen attribute table, adj feature blocks, live parameters, mode and dropout toggles) is a
   rebuilt model or a loud error, never a stale one;
B. one Trainer walked through different shapes, routes, modes and entry points gives, at every call, what a fresh twin gives;
C. the library's per-workspace-pointer forward record follows pointer reuse, out-of-order backwards and eviction, and matcha_backward
   refuses a workspace whose forward was forward_only or already consumed -- before any launch.

Veteran against twin: logits and losses bitwise on every route; gradients and post-AdamW parameters bitwise where the suite already asserts
run-to-run bitwise reproducibility (state_twin.Config.bitwise_tensor), and otherwise against the oracle -- fp64 grade (K = 8) on the
dropout-free steps marked (g), the 1e-4 parity with the kernels' dropout masks injected on the others.  test_two_fresh_twins_agree is the
per-route evidence that a forward is bitwise reproducible by itself.  Nothing here tries to make a kernel fault: every "refused" case is
a host-side state check that returns before a launch, asserted with the launch log.  GPU only (-m gpu).
"""
import copy
import ctypes as C
import io
from dataclasses import dataclass, replace
from typing import FrozenSet

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from oracle import hypersagnn as O
from tests import fp64_grade as G
from tests import state_twin as S
from tests.test_hip_fp64_grade import _ADJ64, _BIG64, _FRONT64, _SMALL, _SORTED_TABLE
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

CONFIGS = {
    "t64": S.Config("table", 64, "hg38_1mb", 201),       # front_fwd3 / front_bwd, attr_mode 1, table padded to 32 floats
    "t128": S.Config("table", 128, "c1", 202, deterministic=False),      # embed_fwd, enc128 (which a deterministic Trainer does not run)
    "a64": S.Config("adj", 64, "c23", 203, deterministic=False),         # fused adj kernels
    "t16": S.Config("table", 16, "tiny", 204),           # layer by layer
}
ROWS_PER_K = {"t64": 256, "t128": 128, "a64": 128, "t16": 64}
_LW = frozenset({"attn_fwd_kernel", "attn_bwd_kernel", "embed_fwd_kernel", "gemm_lds_kernel"})       # layer by layer, with either table gradient
ROUTE = {"t64": _FRONT64, "t128": frozenset({"embed_fwd_kernel", "enc128_fwd_kernel", "enc128_bwd_kernel"}), "a64": _ADJ64, "t16": _LW}
_MASK63 = 0x7FFFFFFFFFFFFFFF


def _build(cfg, attr=None, weight_seed=None):
    """The configuration's model with synthetic weights (optionally another frozen table / another weight seed), in train mode."""
    own = O.attribute_table(cfg.num)
    sd = synth.make_state_dict(np.random.default_rng(cfg.seed if weight_seed is None else weight_seed), cfg.num, cfg.d, cfg.mode, own)
    if attr is not None:
        for k in list(sd):
            if k.startswith("attribute_dict"):
                sd[k] = attr
    clf, _ = hip_model(cfg.num, cfg.d, cfg.mode, cfg.seed, sd=sd)
    clf.train()
    return clf


def _batch(cfg, name, seed=1):
    x, y, w = G.make_case_batch(cfg.layout, [2, 3, 4, 5], ROWS_PER_K[name], seed)
    return S.dev_batch(x, y, w)


def _trainer(clf, cfg, **kw):
    from matcha_amd.engine import Trainer
    return Trainer(clf, lr=1e-3, deterministic=cfg.deterministic, **kw)


def _autograd_seed(seed_counter):
    return (int(torch.initial_seed()) * 1000003 + seed_counter) & _MASK63


# =================================================================================================================================
# the premise: a forward is bitwise reproducible by itself on every route
# =================================================================================================================================
@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_fresh_twins_agree(name):
    """Two fresh models from one state make the same eval call and the same dropout-on training step: logits and losses bitwise on every
    route (what "logits bitwise" in this module rests on), gradients bitwise where Config.bitwise_tensor says so."""
    cfg = CONFIGS[name]
    st = S.model_state(_build(cfg))
    batch = _batch(cfg, name)
    outs = []
    for _ in range(2):
        clf = S.fresh_model(cfg, st)
        np.random.seed(3)
        outs.append((S.eval_call(clf, batch[0]), S.train_call(clf, _trainer(clf, cfg), batch, chrom=1, optimizer=False)))
    S.assert_twin(f"{name} eval", outs[0][0], outs[1][0], cfg)
    S.assert_twin(f"{name} step", outs[0][1], outs[1][1], cfg)


# =================================================================================================================================
# A. a mutated model is a rebuilt model (or a loud error), never a stale one
# =================================================================================================================================
def _veteran_then_twin(label, cfg, clf, batch, must=(), must_not=(), old_trainer=None, attr_mode=None):
    """The next eval logits and the next (dropout-on) training step of the veteran ``clf`` -- on a NEW Trainer -- against the fresh twin
    of its present state and against the oracle on that state at TOL.  ``old_trainer``: a Trainer built before the mutation, which must
    refuse both of its entry points."""
    xd, yd, wd = batch
    not_refused = []                                     # asserted at the end, so that a stale result is reported before a missing refusal
    if old_trainer is not None:
        for what, call in (("forward_backward", lambda: old_trainer.forward_backward(xd, yd, wd, 1.0, 0.001, 1)),
                           ("eval_forward", lambda: old_trainer.eval_forward(xd, yd, wd, 1))):
            try:
                call()
            except _lib.MatchaHipError as e:
                assert "create a new Trainer" in str(e), e
            else:
                not_refused.append(what)
    st = S.model_state(clf)

    def calls(m):
        np.random.seed(11)                               # the adj front end draws its eval-time reconstruction chromosome from numpy
        ev = S.eval_call(m, xd)
        return ev, S.train_call(m, _trainer(m, cfg), batch, 1.0, 0.001, 1, optimizer=False)

    with _lib.launch_log() as log:
        ev, out = calls(clf)
    ran = S.ran_kernels(log)
    if attr_mode is not None:
        assert clf._runtime().attr_mode == attr_mode, (label, "attr_mode", clf._runtime().attr_mode)
    ev2, out2 = calls(S.fresh_model(cfg, st))
    S.assert_twin(label + " eval", ev, ev2, cfg)
    S.assert_twin(label + " step", out, out2, cfg)
    e_ev, _ = S.oracle_parity(label + " eval", cfg, st, batch, ev, backward=False)
    masks = S.call_masks(cfg, clf, 1, xd.numel())       # a new Trainer's seed cell is 0 and is advanced before the step
    e_tr, _ = S.oracle_parity(label + " step", cfg, st, batch, out, alpha=1.0, beta=0.001, chrom=1, masks=masks)
    S.assert_kernels(label, ran, must, must_not)
    assert not not_refused, (label, "the Trainer built before the change went on without raising", not_refused)
    print(f"{label}: kernels {sorted(ran)}: twin bitwise, oracle eval {e_ev:.1e} step {e_tr:.1e}")


def _first_calls(clf, cfg, batch):
    """One eval model(x) and one training step: the model's runtime and a Trainer now exist and have been used."""
    np.random.seed(5)
    S.eval_call(clf, batch[0])
    tr = _trainer(clf, cfg)
    S.train_call(clf, tr, batch, 1.0, 0.001, 2)
    return tr


def _tables(cfg, scenario):
    """(table before, table after, attr_mode expected after)."""
    own, other = O.attribute_table(cfg.num), O.attribute_table(S.other_num(cfg.num))
    dense = np.random.default_rng(17).normal(size=own.shape).astype(np.float32)
    dense[0] = 0.0                                       # row 0 is the padding row (main.py:508)
    return {"structured_to_structured": (own, other, 1), "structured_to_dense": (own, dense, 0), "dense_to_structured": (dense, other, 1)}[scenario]


def _set_table(clf, how, new):
    new = torch.from_numpy(new)
    if how == "load_state_dict":                         # in-place copy_ into the frozen weight: same pointer, version bump
        sd = {k: v.detach().clone() for k, v in clf.state_dict().items()}
        for k in sd:
            if k.startswith("attribute_dict"):
                sd[k] = new
        clf.load_state_dict(sd)
    elif how == "copy_":
        with torch.no_grad():
            clf.attribute_dict_embedding.weight.copy_(new.cuda())
    else:                                                # a new Parameter: the pointer moves
        clf.attribute_dict_embedding.weight = torch.nn.Parameter(new.cuda(), requires_grad=False)


@pytest.mark.parametrize("scenario", ["structured_to_structured", "structured_to_dense", "dense_to_structured"])
@pytest.mark.parametrize("how", ["load_state_dict", "copy_", "assign"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_frozen_attribute_table_changed_after_first_forward(name, how, scenario):
    """A.1 + A.3: the frozen table really changes (same shape) after the model's first forward and first training step.  The runtime's
    padded copy, attr_mode, attr_bounds and attr_scale must follow -- another structured table has other bounds and another scale, a dense
    table must drop to the gathering path, a structured one after a dense one must be recognised -- and the Trainer built before the
    change must refuse to go on; a new one matches the twin and the oracle."""
    cfg = CONFIGS[name]
    before, after, mode_after = _tables(cfg, scenario)
    clf = _build(cfg, attr=before)
    batch = _batch(cfg, name)
    tr = _first_calls(clf, cfg, batch)
    assert clf._runtime().attr_mode == (0 if scenario == "dense_to_structured" else 1)
    _set_table(clf, how, after)
    must, must_not = ROUTE[name], ()
    if name == "t64" and mode_after == 0:
        must, must_not = {"front_fwd_kernel", "front_bwd_kernel"}, {"front_fwd3_kernel"}
    _veteran_then_twin(f"{name} {how} {scenario}", cfg, clf, batch, must, must_not, old_trainer=tr, attr_mode=mode_after)


class _CountEqual:
    """torch.equal with a counter that runs while ``on``: the runtime's only device compare is the one of still_packed()."""

    def __init__(self, monkeypatch):
        self.n, self.on, self.real = 0, False, torch.equal
        monkeypatch.setattr(torch, "equal", self)

    def __call__(self, a, b):
        self.n += 1 if self.on else 0
        return self.real(a, b)

    def __enter__(self):
        self.on = True

    def __exit__(self, *a):
        self.on = False


@pytest.mark.parametrize("name", list(CONFIGS))
def test_same_bytes_reloaded_keeps_the_runtime_and_the_trajectory(name, monkeypatch):
    """A.2: load_state_dict of the model's own bytes (what train() does at the end of every phase) bumps the frozen table's version and
    nothing else: the runtime is not rebuilt, the Trainer keeps stepping, and 3 steps + reload + 3 steps give the trajectory of a Trainer
    that never saw a reload -- bitwise where steps are bitwise reproducible, step against fresh twin elsewhere.  still_packed() compares
    integers: no device compare on a plain step, exactly one per version bump."""
    cfg = CONFIGS[name]
    clf, control = _build(cfg), _build(cfg)
    tr, ctr = _trainer(clf, cfg, base_seed=5), _trainer(control, cfg, base_seed=5)
    batches = [_batch(cfg, name, seed=10 + i) for i in range(3)]
    bitwise = cfg.bitwise_tensor("node_embedding.weight")
    counter = _CountEqual(monkeypatch)
    rt = clf._runtime()

    def three_steps(tag):
        for i, b in enumerate(batches):
            if not bitwise:
                ms, ts = S.model_state(clf), S.trainer_state(tr)
            with counter:
                out = S.train_call(clf, tr, b, chrom=i)
            if bitwise:
                S.assert_twin(f"{name} {tag} step {i}", out, S.train_call(control, ctr, b, chrom=i), cfg, everything=True)
            else:
                twin = S.fresh_model(cfg, ms)
                S.assert_twin(f"{name} {tag} step {i}", out, S.train_call(twin, S.fresh_trainer(twin, ts), b, chrom=i), cfg)

    three_steps("before")
    assert counter.n == 0, counter.n
    for reload in (1, 2):
        clf.load_state_dict({k: v.detach().clone() for k, v in clf.state_dict().items()})
        with counter:
            assert clf._runtime() is rt                  # same bytes: no rebuild ...
            assert rt.still_packed()
        assert counter.n == reload, counter.n             # ... decided by ONE compare per version bump
        three_steps(f"after reload {reload}")
        assert counter.n == reload, counter.n
    if bitwise:
        for a, b in ((tr.exp_avg, ctr.exp_avg), (tr.exp_avg_sq, ctr.exp_avg_sq), (tr.seg_step, ctr.seg_step), (tr.seed, ctr.seed)):
            assert counter.real(a, b)
    print(f"{name}: 9 steps across 2 same-byte reloads, runtime kept, {counter.n} device compares: "
          f"{'bitwise the never-reloaded trajectory' if bitwise else 'every step bitwise its fresh twin (logits, losses)'}")


@pytest.mark.parametrize("what", ["feature_block_assigned", "feature_block_copy_", "inter_assigned", "inter_copy_"])
def test_adj_frozen_inputs_changed_after_first_forward(what):
    """A.4: the reference reads embeddings[i].embedding and inter_initial.embedding on every forward; the runtime holds a re-packed copy
    of the feature blocks.  One block / inter_initial replaced after the first forward, by a new tensor and in place."""
    cfg = CONFIGS["a64"]
    clf = _build(cfg)
    batch = _batch(cfg, "a64")
    tr = _first_calls(clf, cfg, batch)
    ne = clf.node_embedding
    holder = ne.embeddings[2] if what.startswith("feature") else ne.inter_initial
    old = holder.embedding
    new = (old.flip(0) * 0.5 + 0.25 * old.roll(1, 1)).contiguous()
    assert new.shape == old.shape and not torch.equal(new, old)
    if what.endswith("assigned"):
        holder.embedding = new
    else:
        holder.embedding.copy_(new)
    _veteran_then_twin(f"a64 {what}", cfg, clf, batch, ROUTE["a64"], old_trainer=tr)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_other_weights_loaded_after_first_forward(name):
    """A.5: load_state_dict of different weights goes in place into the flat views: no rebuild, the kernels see the new values, the
    Trainer built before keeps working (its moments kept) and matches its twin."""
    cfg = CONFIGS[name]
    clf = _build(cfg)
    batch = _batch(cfg, name)
    tr = _first_calls(clf, cfg, batch)
    rt = clf._runtime()
    donor = S.model_state(_build(cfg, weight_seed=cfg.seed + 1))
    clf.load_state_dict(donor["sd"])
    assert clf._runtime() is rt
    for k, v in clf.state_dict().items():
        assert torch.equal(v, donor["sd"][k]), k
    ms, ts = S.model_state(clf), S.trainer_state(tr)
    out = S.train_call(clf, tr, batch, chrom=1)
    twin = S.fresh_model(cfg, ms)
    S.assert_twin(f"{name} old Trainer after load_state_dict", out, S.train_call(twin, S.fresh_trainer(twin, ts), batch, chrom=1), cfg)
    _veteran_then_twin(f"{name} other weights", cfg, clf, batch, ROUTE[name])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_moved_parameters_rebuild_the_runtime_and_noops_do_not(name):
    """A.5: p.data = p.data.clone() on two parameters moves their storage: rebuild, values kept, the old Trainer refuses.  model.to("cuda")
    and model.float() on a float32 model on the device are no-ops: same runtime, the Trainer goes on."""
    cfg = CONFIGS[name]
    clf = _build(cfg)
    batch = _batch(cfg, name)
    tr = _first_calls(clf, cfg, batch)
    rt = clf._runtime()
    assert clf.to("cuda") is clf and clf.float() is clf
    assert clf._runtime() is rt
    ms, ts = S.model_state(clf), S.trainer_state(tr)
    out = S.train_call(clf, tr, batch, chrom=1)
    twin = S.fresh_model(cfg, ms)
    S.assert_twin(f"{name} after .to() / .float()", out, S.train_call(twin, S.fresh_trainer(twin, ts), batch, chrom=1), cfg)
    before = S.model_state(clf)["sd"]
    for p in (clf.attribute_nn.weight, clf.encode1.mul_head_attn.w_qs.weight):
        p.data = p.data.clone()
    rt2 = clf._runtime()
    assert rt2 is not rt
    for k, v in clf.state_dict().items():
        assert torch.equal(v, before[k]), k
    _veteran_then_twin(f"{name} moved parameters", cfg, clf, batch, ROUTE[name], old_trainer=tr)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_deepcopy_after_training_steps_trains_independently(name):
    """A.5: copy.deepcopy(model) after Trainer steps: copy and original then train independently, each bitwise its twin, neither sees the
    other's updates."""
    cfg = CONFIGS[name]
    clf = _build(cfg)
    batch, batch2 = _batch(cfg, name), _batch(cfg, name, seed=2)
    tr = _first_calls(clf, cfg, batch)
    dup = copy.deepcopy(clf)
    assert dup._runtime() is not clf._runtime() and dup._runtime().flat.data_ptr() != clf._runtime().flat.data_ptr()
    st = S.model_state(clf)
    for k, v in dup.state_dict().items():
        assert torch.equal(v, st["sd"][k]), k
    ts = S.trainer_state(tr)
    tr_dup = _trainer(dup, cfg, base_seed=9)
    ts_dup = S.trainer_state(tr_dup)
    out_dup = S.train_call(dup, tr_dup, batch2, chrom=1)                 # the copy steps first ...
    for k, v in clf.state_dict().items():
        assert torch.equal(v, st["sd"][k]), (k, "the original saw the copy's update")
    out = S.train_call(clf, tr, batch, chrom=1)                          # ... then the original, on another batch
    for n, p in dup.named_parameters():
        assert torch.equal(p, out_dup["param/" + n]), (n, "the copy saw the original's update")
    twin = S.fresh_model(cfg, st)
    S.assert_twin(f"{name} original after deepcopy", out, S.train_call(twin, S.fresh_trainer(twin, ts), batch, chrom=1), cfg)
    twin = S.fresh_model(cfg, st)
    S.assert_twin(f"{name} deepcopy", out_dup, S.train_call(twin, S.fresh_trainer(twin, ts_dup), batch2, chrom=1), cfg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pickled_model_after_trainer_steps_and_late_state_dict(name):
    """A.5: torch.save(model) / torch.load after Trainer steps gives bitwise the original's eval logits; a state_dict() taken BEFORE a step
    aliases the live values after it, as in torch (the reference's checkpoint code reads it late)."""
    cfg = CONFIGS[name]
    clf = _build(cfg)
    batch = _batch(cfg, name)
    tr = _first_calls(clf, cfg, batch)
    sd_early = clf.state_dict()
    frozen_before = {k: v.detach().clone() for k, v in sd_early.items()}
    S.train_call(clf, tr, batch, chrom=1)
    names = {id(p): n for n, p in clf.named_parameters()}
    live = {names[id(p)] for p in clf._runtime().live}
    changed = 0
    for k, v in sd_early.items():
        now = clf.state_dict()[k]
        assert v.data_ptr() == now.data_ptr() and torch.equal(v, now), (k, "an early state_dict() no longer aliases the live value")
        changed += int(k in live and not torch.equal(v, frozen_before[k]))
    assert changed >= 20, changed                         # the step did move the live parameters the early dict shows
    buf = io.BytesIO()
    torch.save(clf, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    np.random.seed(4)
    a = S.eval_call(clf, batch[0])
    np.random.seed(4)
    b = S.eval_call(loaded, batch[0])
    S.assert_twin(f"{name} unpickled model", a, b, cfg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_mode_and_dropout_toggles_take_effect_on_the_next_call(name):
    """A.6: train() / eval() and a changed Dropout.p are read per call.  model(x) in eval mode, in train mode, with another p, with p = 0,
    in eval mode again -- each against the oracle with exactly the masks that call must draw (none in eval mode); then the Trainer the same
    way: a default step, a step under model.eval() (no dropout), a step with another p."""
    cfg = CONFIGS[name]
    clf = _build(cfg)
    batch = _batch(cfg, name)
    xd = batch[0]
    st = S.model_state(clf)
    defaults = list(st["drop"])
    n_tok = xd.numel()

    def forward(label, training, ps):
        clf.train(training)
        S.set_dropout(clf, ps)
        rt = clf._runtime()
        c0 = rt.seed_counter
        np.random.seed(2)
        with torch.no_grad():
            out = {"logits": clf(xd).reshape(-1).clone()}
        masks = S.call_masks(cfg, clf, _autograd_seed(rt.seed_counter), n_tok)
        assert (rt.seed_counter == c0) == (masks is None), label
        e, _ = S.oracle_parity(f"{name} {label}", cfg, st, batch, out, backward=False, masks=masks)
        return out["logits"], e

    e0, err0 = forward("eval", False, defaults)
    t1, err1 = forward("train", True, defaults)
    t2, err2 = forward("train p=0.1", True, 0.1)
    t3, err3 = forward("train p=0", True, 0.0)
    e1, err4 = forward("eval again", False, defaults)
    assert torch.equal(e0, e1)
    assert not torch.equal(e0, t1) and not torch.equal(t1, t2) and not torch.equal(t2, t3)
    tr = _trainer(clf, cfg, base_seed=3)
    errs = []
    for i, (label, training, ps) in enumerate((("step", True, defaults), ("step in eval mode", False, defaults), ("step p=0.1", True, 0.1))):
        clf.train(training)
        S.set_dropout(clf, ps)
        ms, seed = S.model_state(clf), int(tr.seed) + 1
        out = S.train_call(clf, tr, batch, chrom=i)
        e, _ = S.oracle_parity(f"{name} {label}", cfg, ms, batch, out, chrom=i, masks=S.call_masks(cfg, clf, seed, n_tok))
        errs.append(e)
    print(f"{name}: forward vs oracle {err0:.1e} {err1:.1e} {err2:.1e} {err3:.1e} {err4:.1e}; steps {errs[0]:.1e} {errs[1]:.1e} {errs[2]:.1e}")


# =================================================================================================================================
# B. history independence of the calls on one Trainer / model
# =================================================================================================================================
@dataclass
class Step:
    label: str
    kind: str                              # train | eval | eval_forward | embed | autograd | second_trainer
    batch: tuple                           # (x, y, w) numpy
    grade: bool = False                    # (g): dropout off for this call, held to fp32 grade
    option: str = ""                       # library switch the call (and its twin's) runs under
    lif: bool = True                       # Trainer.loss_in_forward
    alpha: float = 1.0
    beta: float = 0.001
    chrom: int = 0
    bad_ids: bool = False                  # the batch holds out-of-range ids: flagged, read as padding
    must: FrozenSet[str] = frozenset()
    must_not: FrozenSet[str] = frozenset()


def _do(s: Step, i, clf, tr, cfg):
    xd, yd, wd = S.dev_batch(*s.batch)
    np.random.seed(100 + i)
    with S.option(s.option):
        if s.kind == "train":
            return S.train_call(clf, tr, (xd, yd, wd), s.alpha, s.beta, s.chrom)
        if s.kind == "eval":
            return S.eval_call(clf, xd)
        if s.kind == "eval_forward":
            lg = tr.eval_forward(xd, yd, wd, s.chrom)
            out = {"logits": lg.clone(), "losses": tr.losses.clone()}
        elif s.kind == "embed":
            with torch.no_grad():
                dyn, sta, attn = clf.get_embedding(xd)
                out = {"dynamic": dyn.clone(), "static": sta.clone(), "attn": attn.clone(), "node": clf.get_node_embeddings(xd).clone()}
        elif s.kind == "autograd":
            before = tr.gflat.clone()
            out = S.autograd_call(clf, xd, weight=wd)
            assert torch.equal(before, tr.gflat), "the autograd route wrote into the Trainer's gradient buffer"
        elif s.kind == "second_trainer":
            out = S.train_call(clf, _trainer(clf, cfg, base_seed=99), (xd, yd, wd), s.alpha, s.beta, s.chrom, optimizer=False)
        else:
            raise AssertionError(s.kind)
    torch.cuda.synchronize()
    return out


def _seg_names(clf, tr):
    names = {id(p): n for n, p in clf.named_parameters()}
    return [names[id(p)] for p in tr.rt.live]


def _run_steps(name, cfg, steps, clf=None, tr=None):
    """Walk one Trainer through ``steps``; every call against the fresh twin of the state right before it."""
    clf = _build(cfg) if clf is None else clf
    tr = _trainer(clf, cfg, base_seed=7) if tr is None else tr
    atomics = not cfg.bitwise_tensor("node_embedding.weight")        # some gradient goes through float atomics: those go to the oracle
    opt, dummy = O.AdamWRef(), None
    for i, s in enumerate(steps):
        label = f"{name}[{i + 1}: {s.label}]"
        tr.loss_in_forward = s.lif
        old_p = S.set_dropout(clf, 0.0) if s.grade else None
        ms, ts = S.model_state(clf), S.trainer_state(tr)
        with _lib.launch_log() as log:
            out = _do(s, i, clf, tr, cfg)
        ran = S.ran_kernels(log)
        if s.bad_ids:
            with pytest.raises(IndexError):
                tr.check_status()
        tr.check_status()                                 # silent: raised once, or nothing to raise
        twin = S.fresh_model(cfg, ms)
        out2 = _do(s, i, twin, S.fresh_trainer(twin, ts), cfg)
        # the autograd route has no deterministic switch: its front-end gradients are float atomics whatever the Trainer's flag says
        S.assert_twin(label, out, out2, replace(cfg, deterministic=False) if s.kind == "autograd" else cfg)
        how = "bitwise"
        x, y, w = s.batch
        ob = S.dev_batch(x, y, w)
        ref_grads = None
        if s.bad_ids:
            # the reference raises on such a batch (nn.Embedding) and so does check_status() above: there is no oracle answer to hold the
            # flagged step to -- it is held to its twin, and the clean step behind it to twin and oracle
            how = "bitwise (flagged batch: IndexError raised once, no oracle)"
        elif s.kind == "train" and s.grade:
            ratio, ref = S.fp64_grade(label, cfg, ms, ob, out, alpha=s.alpha, beta=s.beta, chrom=s.chrom)
            how = f"bitwise, fp64 grade worst e/noise {ratio:.2f}"
            ref_grads = {n: (None if g is None else torch.zeros(1)) for n, g in ref.r64.grads.items()}
        elif s.kind == "train" and atomics:
            masks = S.call_masks(cfg, clf, int(ts["seed"]) + 1, x.size)
            e, grads = S.oracle_parity(label, cfg, ms, ob, out, alpha=s.alpha, beta=s.beta, chrom=s.chrom, masks=masks)
            how = f"logits / losses bitwise, gradients vs oracle {e:.1e}"
            ref_grads = {n: (None if g is None else torch.zeros(1)) for n, g in grads.items()}
        elif s.kind == "autograd":
            masks = S.call_masks(cfg, clf, _autograd_seed(ms["seed_counter"] + 1), x.size)
            e, _ = S.oracle_parity(label, cfg, ms, ob, out, chrom=0, masks=masks, dlogits=ob[2])
            how = f"logits bitwise, gradients vs oracle {e:.1e}"
        if cfg.mode == "adj" and s.kind == "train":
            # AdamW must skip exactly the reference's grad-None tensors: per-tensor step counts of AdamWRef driven by the oracle's sets
            dummy = dummy or {n: torch.zeros(1) for n in ref_grads}
            opt.step(dummy, ref_grads)
            want = [opt.state.get(n, {"step": 0})["step"] for n in _seg_names(clf, tr)]
            assert tr.seg_step.cpu().tolist() == want, (label, "seg_step", tr.seg_step.cpu().tolist(), want)
        S.assert_kernels(label, ran, s.must, s.must_not)
        print(f"{label}: B = {len(x)}, L = {x.shape[1]}, kernels {sorted(ran)}: {how}")
        if old_p is not None:
            S.set_dropout(clf, old_p)
    return clf, tr


def _step_outputs(clf, tr, logits):
    out = {"logits": logits.clone(), "losses": tr.losses.clone(), "seg_step": tr.seg_step.clone()}
    for n, p in clf.named_parameters():
        out["param/" + n] = p.detach().clone()
    torch.cuda.synchronize()
    return out


def _captured_block(name, cfg, clf, tr, captured, other, same_shape, beta=0.0):
    """B.15: capture() on static buffers, then replay, one eager step of another shape, one eager step of the captured shape, replay again
    -- against the same four steps run eagerly by a twin loaded with the veteran's state as it is when capture() returns (its two warm-up
    steps are real steps).  Where a step is not bitwise reproducible (float atomics) logits, losses and seg_step are still bitwise, the
    parameters the step leaves are held to the twin's to rounding (state_twin.assert_params_to_rounding: what a replay or an eager step
    WRITES is compared, not only what it returns), and only then is the twin re-loaded with the veteran's state, so that the next call
    is again compared from identical inputs."""
    cell = torch.zeros(1, dtype=torch.int32, device="cuda") if cfg.mode == "adj" else None
    sx, sy, sw = (t.clone() for t in S.dev_batch(*captured))
    chroms = [3, 7, 11, 2]
    if cell is not None:
        cell.fill_(1)
    replay = tr.capture(sx, sy, sw, 1.0, beta, cell if cell is not None else 0)
    ms, ts = S.model_state(clf), S.trainer_state(tr)
    twin = S.fresh_model(cfg, ms)
    ttr = S.fresh_trainer(twin, ts)
    tcell = torch.zeros(1, dtype=torch.int32, device="cuda") if cell is not None else None
    bitwise = cfg.bitwise_tensor("node_embedding.weight")
    for j, (what, b) in enumerate((("replay", captured), ("eager, another shape", other), ("eager, the captured shape", same_shape), ("replay again", captured))):
        label = f"{name}[capture {j + 1}: {what}]"
        xd, yd, wd = S.dev_batch(*b)
        for c in (cell, tcell):
            if c is not None:
                c.fill_(chroms[j])
        with _lib.launch_log() as log:
            if what.startswith("replay"):
                sx.copy_(xd), sy.copy_(yd), sw.copy_(wd)
                _, _, lg = replay()
            else:
                _, _, lg = tr.step(xd, yd, wd, 1.0, beta, cell if cell is not None else 0)
            out = _step_outputs(clf, tr, lg)
        _, _, lg2 = ttr.step(xd, yd, wd, 1.0, beta, tcell if tcell is not None else 0)
        out2 = _step_outputs(twin, ttr, lg2)
        S.assert_twin(label, out, out2, cfg)
        if what.startswith("replay"):
            assert not S.ran_kernels(log), (label, "a replay launches nothing through the library's launch sites")
        how = "bitwise (logits, losses, parameters)"
        if not bitwise:
            med, mx = S.assert_params_to_rounding(label, out, out2, cfg, tr.lr)
            how = f"logits / losses bitwise, atomics-fed parameters to rounding (median {med:.1e}, max {mx:.1e})"
            twin.load_state_dict(S.model_state(clf)["sd"])
            S.load_trainer_state(ttr, S.trainer_state(tr))
        print(f"{label}: B = {len(xd)}, L = {xd.shape[1]}: {how}")


def _with_padding_rows(batch, frac, seed):
    x, y, w = (a.copy() for a in batch)
    rows = np.random.default_rng(seed).permutation(len(x))[: int(frac * len(x))]
    x[rows] = 0
    return x, y, w


def _table_steps(cfg, rows_per_k):
    """The sixteen-point script of the table front end (rows_per_k = 1024: 4 096-row batches)."""
    lay = cfg.layout
    N = cfg.n_nodes
    r7 = max(1, (4 * rows_per_k) // 7)
    b1 = G.make_case_batch(lay, [2, 3, 4, 5], rows_per_k, 301)
    b3 = G.make_case_batch(lay, [2, 3, 4, 5], rows_per_k, 303)
    small = tuple(a[:3] for a in G.make_case_batch(lay, [2, 3, 4, 5], 4, 302))
    k2 = G.make_case_batch(lay, [2], 4 * rows_per_k, 305, L=5)
    pad = _with_padding_rows(G.make_case_batch(lay, [2, 3, 4, 5], rows_per_k, 306), 0.10, 6)
    l8 = G.make_case_batch(lay, [2, 3, 4, 5, 6, 7, 8], r7, 307, L=8)
    big = cfg.d == 64 and rows_per_k >= 1024
    fused_train = (_BIG64 | _FRONT64 | (_SORTED_TABLE if cfg.deterministic else frozenset())) if big else frozenset()
    not_small = (_SMALL | {"attn_fwd_kernel"}) if big else frozenset()
    steps = [
        Step("train, k in 2..5 (g)", "train", b1, grade=True, must=fused_train, must_not=not_small),
        Step("train, 3 rows", "train", small, must=(_SMALL | _FRONT64 | {"fused_bwdh_kernel"}) if cfg.d == 64 else frozenset(),
             must_not={"fused_fwd32_kernel", "tail_bwd64_kernel"}),
        Step("model(x) eval", "eval", b3, must={"fused_fwd32_kernel", "front_fwd3_kernel"} if big else frozenset(),
             must_not={"fused_bwdh_kernel", "front_bwd_kernel", "enc128_bwd_kernel", "attn_bwd_kernel"}),
        Step("train, step 1's batch again", "train", b1, chrom=1, must=fused_train, must_not=not_small),
        Step("train, all k = 2", "train", k2, chrom=2, must=fused_train, must_not=not_small),
        Step("train, 10 % all-padding rows", "train", pad, chrom=3, must=fused_train, must_not=not_small),
        Step("train, step 1's batch again", "train", b1, chrom=4, must=fused_train, must_not=not_small),
        Step("train, L = 8, k in 2..8", "train", l8, chrom=5, must=fused_train, must_not=not_small),
        Step("train, L = 5 again (g)", "train", b3, grade=True, chrom=6, must=fused_train, must_not=not_small),
    ]
    if cfg.d == 64:
        e_minus = tuple(a[: G.edge_rows("edge-", 5)] for a in b3)
        e_plus = tuple(a[: G.edge_rows("edge+", 5)] for a in b1)
        assert len(e_plus[0]) == len(e_minus[0]) + 1
        steps += [
            Step("train, edge- rows", "train", e_minus, chrom=7, must={"fused_fwd32h_kernel", "fused_bwdh_kernel"} | _FRONT64,
                 must_not={"fused_fwd32_kernel", "tail_bwd64_kernel"}),
            Step("train, edge+ rows", "train", e_plus, chrom=8, must=_BIG64 | _FRONT64, must_not=_SMALL),
        ]
    emb = tuple(a[:300] for a in b3)
    steps += [
        Step("get_embedding + get_node_embeddings, 300 rows", "embed", emb, must={"ln3_fwd_kernel"}, must_not={"fused_fwd32_kernel", "fused_fwd32h_kernel", "enc128_fwd_kernel"}),
        Step("train, step 1's batch again", "train", b1, chrom=9, must=fused_train, must_not=not_small),
    ]
    if cfg.d != 64:
        return steps
    bad = tuple(a.copy() for a in b3)
    bad[0][5, 1], bad[0][77, 0] = N + 9, 10 ** 12
    steps += [
        Step("Trainer.eval_forward", "eval_forward", b1, must={"fused_fwd32_kernel", "front_fwd3_kernel"}, must_not={"fused_bwdh_kernel", "front_bwd_kernel"}),
        Step("train, same (B, L)", "train", b3, chrom=10, must=fused_train, must_not=not_small),
        Step("train under disable_fused", "train", b1, option="disable_fused", chrom=11, must=_LW, must_not=_BIG64 | _FRONT64 | _SMALL),
        Step("train", "train", b1, chrom=12, must=fused_train, must_not=not_small),
        Step("train under disable_merged", "train", b1, option="disable_merged", chrom=13, must=_LW, must_not=_BIG64 | _FRONT64 | _SMALL),
        Step("train", "train", b1, chrom=14, must=fused_train, must_not=not_small),
        Step("train, loss_in_forward off", "train", b3, lif=False, chrom=15, must=(fused_train - {"tail_bwd64_kernel"}) | {"head_bwd_kernel"},
             must_not={"tail_bwd64_kernel"}),
        Step("train, loss_in_forward on", "train", b3, chrom=16, must=fused_train, must_not={"head_bwd_kernel"}),
        Step("autograd model(x) + backward", "autograd", b1, must={"fused_bwdh_kernel", "head_bwd_kernel"}, must_not={"tail_bwd64_kernel"}),
        Step("train after the autograd call", "train", b1, chrom=17, must=fused_train, must_not=not_small),
        Step("train, two out-of-range ids", "train", bad, bad_ids=True, chrom=18, must=fused_train),
        Step("train, clean batch", "train", b3, chrom=19, must=fused_train, must_not=not_small),
        Step("a second Trainer's forward_backward", "second_trainer", b1, chrom=20, must=fused_train),
        Step("train, the first Trainer again", "train", b1, chrom=21, must=fused_train, must_not=not_small),
    ]
    return steps


@pytest.mark.parametrize("deterministic", [True, False])
def test_table_d64_call_sequence_is_history_independent(deterministic):
    """B, table front end, embed_dim 64, hg38 1 Mb: points 1-14 and 16 as one walk of one Trainer, then point 15 (capture).  With
    deterministic=True everything is bitwise the twin's; with the default float atomics the front-end gradients of every step go to the
    oracle instead (dropout masks injected) and everything else stays bitwise."""
    cfg = replace(CONFIGS["t64"], deterministic=deterministic)
    name = "t64 det" if deterministic else "t64 atomics"
    clf, tr = _run_steps(name, cfg, _table_steps(cfg, 1024))
    lay = cfg.layout
    _captured_block(name, cfg, clf, tr, G.make_case_batch(lay, [2, 3, 4, 5], 128, 311), G.make_case_batch(lay, [2, 3, 4, 5, 6, 7, 8], 64, 312, L=8),
                    G.make_case_batch(lay, [2, 3, 4, 5], 128, 313))


def _avoiding(cfg, chroms, rows, seed):
    """A batch whose rows avoid the chromosomes ``chroms`` entirely."""
    x, y, w = G.make_case_batch(cfg.layout, [2, 3, 4, 5], 4 * rows, seed)
    n2c = synth.node2chrom(cfg.num)
    keep = ~np.isin(n2c[x], list(chroms)).any(axis=1)
    assert keep.sum() >= 4 * rows, keep.sum()
    return x[keep][: 4 * rows], y[keep][: 4 * rows], w[keep][: 4 * rows]


def test_adj_d64_call_sequence_is_history_independent():
    """B, adj front end, embed_dim 64, c23: points 1-8, 10, 11, 15 with random_chrom changing every step (an int; the device cell in the
    captured part), beta alternating between 0.001 and 0, and two batches whose rows avoid three chromosomes followed by one that has them
    again (the touched flags, per-chromosome seg_step: AdamW must skip exactly the reference's grad-None tensors).  The adj weight
    gradients are float atomics: logits and losses bitwise, every step's gradients against the oracle, seg_step exactly AdamWRef's."""
    cfg, name = CONFIGS["a64"], "a64"
    lay = cfg.layout
    b1 = G.make_case_batch(lay, [2, 3, 4, 5], 1024, 401)
    b3 = G.make_case_batch(lay, [2, 3, 4, 5], 1024, 403)
    small = tuple(a[:3] for a in G.make_case_batch(lay, [2, 3, 4, 5], 4, 402))
    k2 = G.make_case_batch(lay, [2], 4096, 405, L=5)
    pad = _with_padding_rows(G.make_case_batch(lay, [2, 3, 4, 5], 1024, 406), 0.10, 6)
    l8 = G.make_case_batch(lay, [2, 3, 4, 5, 6, 7, 8], 585, 407, L=8)
    av1, av2 = _avoiding(cfg, (0, 5, 22), 256, 408), _avoiding(cfg, (0, 5, 22), 256, 409)
    e_minus = tuple(a[: G.edge_rows("edge-", 5)] for a in b3)
    e_plus = tuple(a[: G.edge_rows("edge+", 5)] for a in b1)
    big = _BIG64 | _ADJ64
    steps = [
        Step("train, k in 2..5 (g)", "train", b1, grade=True, chrom=4, must=big, must_not=_SMALL),
        Step("train, 3 rows", "train", small, beta=0.0, chrom=9, must={"fused_fwd32h_kernel", "adj_fused_fwd_kernel", "adj_fused_bwd_kernel"}, must_not={"fused_fwd32_kernel"}),
        Step("model(x) eval", "eval", b3, must={"fused_fwd32_kernel", "adj_fused_fwd_kernel"}, must_not={"fused_bwdh_kernel", "adj_fused_bwd_kernel"}),
        Step("train, step 1's batch again", "train", b1, chrom=17, must=big, must_not=_SMALL),
        Step("train, all k = 2", "train", k2, beta=0.0, chrom=2, must=big, must_not=_SMALL),
        Step("train, 10 % all-padding rows", "train", pad, chrom=21, must=big, must_not=_SMALL),
        Step("train, step 1's batch again", "train", b1, beta=0.0, chrom=0, must=big, must_not=_SMALL),
        Step("train, rows avoid chromosomes 0, 5, 22", "train", av1, chrom=5, must=_ADJ64),
        Step("train, rows avoid them again", "train", av2, beta=0.0, chrom=12, must=_ADJ64),
        Step("train, every chromosome again", "train", b3, chrom=22, must=big, must_not=_SMALL),
        Step("train, L = 8, k in 2..8", "train", l8, beta=0.0, chrom=13, must=big, must_not=_SMALL),
        Step("train, L = 5 again (g)", "train", b3, grade=True, chrom=6, must=big, must_not=_SMALL),
        Step("train, edge- rows", "train", e_minus, beta=0.0, chrom=7, must={"fused_fwd32h_kernel", "fused_bwdh_kernel"} | _ADJ64, must_not={"fused_fwd32_kernel", "tail_bwd64_kernel"}),
        Step("train, edge+ rows", "train", e_plus, chrom=8, must=big, must_not=_SMALL),
        Step("Trainer.eval_forward", "eval_forward", b1, chrom=3, must={"fused_fwd32_kernel", "adj_fused_fwd_kernel"}, must_not={"fused_bwdh_kernel", "adj_fused_bwd_kernel"}),
        Step("train, same (B, L)", "train", b3, beta=0.0, chrom=10, must=big, must_not=_SMALL),
        Step("train under disable_fused", "train", b1, option="disable_fused", chrom=11, must={"attn_fwd_kernel", "attn_bwd_kernel"}, must_not=_BIG64 | _ADJ64),
        Step("train", "train", b1, beta=0.0, chrom=14, must=big, must_not=_SMALL),
        Step("train under disable_merged", "train", b1, option="disable_merged", chrom=15, must={"attn_fwd_kernel", "attn_bwd_kernel"}, must_not=_BIG64),
        Step("train", "train", b1, beta=0.0, chrom=16, must=big, must_not=_SMALL),
    ]
    clf, tr = _run_steps(name, cfg, steps)
    assert tr.supports_device_chrom()
    _captured_block(name, cfg, clf, tr, G.make_case_batch(lay, [2, 3, 4, 5], 128, 411), G.make_case_batch(lay, [2, 3, 4, 5, 6, 7, 8], 64, 412, L=8),
                    G.make_case_batch(lay, [2, 3, 4, 5], 128, 413), beta=0.001)


@pytest.mark.parametrize("name", ["t128", "t16"])
def test_other_dims_call_sequence_is_history_independent(name):
    """B, table front end at embed_dim 128 (c1, the fused attention block) and 16 (tiny, layer by layer): points 1-7 and 9 at a quarter
    of the rows."""
    cfg = CONFIGS[name]
    steps = _table_steps(cfg, 256)
    # kernel sets per kind of step, read off the first MI355X run and frozen: a size rule that moves a step to another route fails here
    wide = {"attn_fwd_wide_kernel", "attn_bwd_wide_kernel"}
    enc = {"enc128_fwd_kernel", "enc128_bwd_kernel", "enc128_unfold_kernel"}
    sets = {
        # embed_dim 128: the fused attention block; one to three rows do not fit its records and run the wide layer-by-layer kernels
        "t128": dict(train=(ROUTE["t128"] | enc | {"embed_scatter_kernel", "head_bwd_kernel"}, wide | {"attn_fwd_kernel"}),
                     tiny=(wide | {"embed_fwd_kernel", "embed_scatter_kernel", "ln3_fwd_kernel", "ln3_bwd_kernel"}, enc),
                     eval=({"embed_fwd_kernel", "enc128_fwd_kernel", "head_fwd_kernel"}, wide | {"enc128_bwd_kernel", "head_bwd_kernel"}),
                     embed=({"attn_fwd_wide_kernel", "ln3_fwd_kernel", "embed_fwd_kernel", "gather_rows_kernel"}, enc)),
        # embed_dim 16, deterministic: layer by layer at every size, the table gradient sorted
        "t16": dict(train=(_LW | _SORTED_TABLE | {"ln3_fwd_kernel", "ln3_bwd_kernel", "head_bwd_kernel"}, wide | enc | {"embed_scatter_kernel"}),
                    tiny=(_LW | _SORTED_TABLE | {"ln3_fwd_kernel", "ln3_bwd_kernel", "head_bwd_kernel"}, wide | enc | {"embed_scatter_kernel"}),
                    eval=({"attn_fwd_kernel", "embed_fwd_kernel", "gemm_lds_kernel", "ln3_fwd_kernel", "head_fwd_kernel"}, {"attn_bwd_kernel", "head_bwd_kernel"}),
                    embed=({"attn_fwd_kernel", "ln3_fwd_kernel", "embed_fwd_kernel", "gather_rows_kernel"}, wide)),
    }[name]
    for s in steps:
        kind = s.kind if s.kind != "train" else ("tiny" if len(s.batch[0]) <= 3 else "train")
        s.must, s.must_not = frozenset(sets[kind][0]), frozenset(s.must_not) | frozenset(sets[kind][1])
    _run_steps(name, cfg, steps)


# =================================================================================================================================
# C. the per-pointer forward record
# =================================================================================================================================
C_CFG = S.Config("table", 64, "c23", 205, deterministic=False)       # the autograd route: float atomics in front of the encoder


def _pending_forward(clf, x, weight):
    """model(x) with grad enabled, backward NOT yet run: (logits, the scalar to differentiate)."""
    lg = clf(x)
    return lg, (lg * weight.reshape(lg.shape)).sum()


def _grads_of(clf, lg, scalar):
    live = clf._runtime().live
    names = {id(p): n for n, p in clf.named_parameters()}
    gs = torch.autograd.grad(scalar, live, allow_unused=True)
    out = {"logits": lg.detach().reshape(-1).clone()}
    for p, g in zip(live, gs):
        out["grad/" + names[id(p)]] = None if g is None else g.detach().clone()
    torch.cuda.synchronize()
    return out


def _twin_autograd(cfg, st, seed_counter, x, weight, option=""):
    twin = S.fresh_model(cfg, dict(st, seed_counter=seed_counter))
    with S.option(option):
        lg, sc = _pending_forward(twin, x, weight)
        return _grads_of(twin, lg, sc)


def _oracle_autograd(label, cfg, clf, st, seed_counter, x, weight, got):
    """The autograd call that found the runtime's seed counter at ``seed_counter``, against the oracle at TOL -- every gradient, so that
    the front-end tensors, which go through float atomics on this route and are left out of the bitwise comparison, are held to something."""
    masks = S.call_masks(cfg, clf, _autograd_seed(seed_counter + 1), x.numel())
    zeros = torch.zeros(len(x))
    e, _ = S.oracle_parity(label, cfg, st, (x, zeros, weight), got, masks=masks, dlogits=weight)
    return e


def test_backwards_out_of_forward_order():
    """Forwards A, B, C of three shapes (each clf(x) allocates its own workspace), then backwards in the order B, C, A: each gradient set
    equals that of a twin that made the one forward and the one backward (bitwise behind the front end), and the oracle's (all of it)."""
    cfg = C_CFG
    clf = _build(cfg)
    st = S.model_state(clf)
    bs = [S.dev_batch(*G.make_case_batch(cfg.layout, ks, rows, seed, L)) for ks, rows, seed, L in
          (([2, 3, 4, 5], 1, 501, 0), ([2, 3, 4, 5], 300, 502, 0), ([2, 3, 4, 5, 6, 7, 8], 40, 503, 8))]
    bs[0] = tuple(t[:3] for t in bs[0])
    pending = [_pending_forward(clf, b[0], b[2]) for b in bs]
    errs = []
    for i in (1, 2, 0):
        got = _grads_of(clf, *pending[i])
        S.assert_twin(f"backward of forward {'ABC'[i]}", got, _twin_autograd(cfg, st, st["seed_counter"] + i, bs[i][0], bs[i][2]), cfg)
        errs.append(_oracle_autograd(f"backward of forward {'ABC'[i]}", cfg, clf, st, st["seed_counter"] + i, bs[i][0], bs[i][2], got))
    print("forwards A, B, C then backwards B, C, A: each bitwise its twin (logits, gradients behind the front end), every gradient vs oracle "
          + " ".join(f"{e:.1e}" for e in errs))


class _Pointers:
    """Records the workspace pointers a runtime hands out, per label; optionally serves every request from ONE pre-allocated buffer."""

    def __init__(self, rt, pool=None):
        self.rt, self.pool, self.seen, self.label = rt, pool, {}, None
        self.orig = rt.workspace
        rt.workspace = self

    def nbytes(self, B, L, forward_only=False):
        query = self.rt.lib.matcha_workspace_bytes_forward if forward_only else self.rt.lib.matcha_workspace_bytes
        n = query(C.byref(self.rt.shape), B, L)
        assert n > 0
        return n

    def __call__(self, B, L, forward_only=False):
        ws = self.orig(B, L, forward_only) if self.pool is None else self.pool[: self.nbytes(B, L, forward_only)]
        self.seen.setdefault(ws.data_ptr(), set()).add(self.label)
        return ws


def test_workspace_pointer_reused_by_another_shape_and_route():
    """Forward + backward of shape S1, everything released (no empty_cache), then forward + backward of another shape on ANOTHER route
    (disable_fused flipped), 50 alternations: the caching allocator hands a released workspace's pointer to the next one, and the per-pointer
    record must follow.  Then 10 more alternations with every workspace carved from one pre-allocated buffer, so that the pointer IS shared
    whatever the allocator does (on the MI355X torch's allocator gave each shape its own block: 2 distinct pointers over the 100 pairs, none
    shared -- the second phase is what exercises a pointer changing shape and route).  Every result equals its twin's; the pointer
    statistics are printed."""
    cfg = C_CFG
    clf = _build(cfg)
    st = S.model_state(clf)
    s1 = S.dev_batch(*G.make_case_batch(cfg.layout, [2, 3, 4, 5], 64, 511))
    s2 = S.dev_batch(*G.make_case_batch(cfg.layout, [2, 3, 4, 5, 6, 7, 8], 48, 512, L=8))
    rt = clf._runtime()
    rec = _Pointers(rt)
    counter = st["seed_counter"]
    try:
        for phase, n in (("allocator", 50), ("one buffer", 10)):
            if phase == "one buffer":
                rec.pool = torch.empty(max(rec.nbytes(*s1[0].shape), rec.nbytes(*s2[0].shape)), dtype=torch.uint8, device="cuda")
                rec.seen = {}
            errs = []
            for it in range(n):
                for tag, b, opt, must, must_not in (("S1", s1, "", {"fused_fwd32h_kernel", "fused_bwdh_kernel"}, {"attn_fwd_kernel"}),
                                                    ("S2", s2, "disable_fused", {"attn_fwd_kernel", "attn_bwd_kernel"}, {"fused_fwd32h_kernel", "fused_bwdh_kernel"})):
                    rec.label = tag
                    with S.option(opt), _lib.launch_log() as log:
                        lg, sc = _pending_forward(clf, b[0], b[2])
                        got = _grads_of(clf, lg, sc)
                    del lg, sc
                    counter += 1
                    S.assert_kernels(f"{phase} {it} {tag}", S.ran_kernels(log), must, must_not)
                    S.assert_twin(f"{phase} {it} {tag}", got, _twin_autograd(cfg, st, counter - 1, b[0], b[2], opt), cfg)
                    if it in (0, n - 1):                  # the first and the last pair of a phase also against the oracle, every gradient
                        errs.append(_oracle_autograd(f"{phase} {it} {tag}", cfg, clf, st, counter - 1, b[0], b[2], got))
            shared = sum(1 for v in rec.seen.values() if len(v) == 2)
            print(f"{phase}: {2 * n} forward + backward pairs, {len(rec.seen)} distinct workspace pointers, {shared} of them used by both shapes / routes; "
                  f"vs oracle {max(errs):.1e}")
            if phase == "one buffer":
                assert len(rec.seen) == 1 and shared == 1
    finally:
        rt.workspace = rec.orig


def _refused(call):
    with _lib.launch_log() as log:
        rc = call()
    msg = _lib.load().matcha_last_error().decode()
    assert rc == -22 and "no matcha_forward on record" in msg, (rc, msg)      # MATCHA_EINVAL
    assert not S.ran_kernels(log), sorted(S.ran_kernels(log))                # refused before any launch


def test_backward_refused_after_forward_only_and_after_a_consumed_forward():
    """Through the C ABI on a full-size workspace: a second matcha_backward on a workspace whose forward one backward already consumed, and
    a matcha_backward on a pointer whose last forward was forward_only (it overwrote what the training forward before it had left): both
    refused with MATCHA_EINVAL, a message and no launch.  A fresh forward makes the workspace usable again."""
    cfg = CONFIGS["t64"]
    clf = _build(cfg)
    tr = _trainer(clf, cfg)
    rt, lib = tr.rt, tr.lib
    xd, yd, wd = S.dev_batch(*G.make_case_batch(cfg.layout, [2, 3, 4, 5], 1024, 521))
    B, L = xd.shape
    ws, logits = tr._buffers(B, L)
    opts = tr._opts(1.0, 0.001, 0)
    fo = tr._opts(1.0, 0.001, 0)
    fo.training, fo.forward_only, fo.loss_in_forward = 0, 1, 0

    def forward(o):
        return lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(o), _lib.ptr(xd), B, L, _lib.ptr(yd), _lib.ptr(wd),
                                  _lib.ptr(logits), _lib.ptr(tr.losses), _lib.ptr(ws), ws.numel(), rt.stream())

    def backward():
        return lib.matcha_backward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xd), B, L, _lib.ptr(yd), _lib.ptr(wd),
                                   None, None, C.byref(tr.grads), _lib.ptr(tr.touched), _lib.ptr(ws), ws.numel(), rt.stream())

    _lib.check(forward(opts), "matcha_forward")
    _lib.check(backward(), "matcha_backward")
    first = tr.gflat.clone()
    _refused(backward)                                   # one backward per forward
    assert torch.equal(tr.gflat, first)
    _lib.check(forward(opts), "matcha_forward")
    _lib.check(forward(fo), "matcha_forward")            # forward_only on the pointer that held a training forward
    _refused(backward)
    assert torch.equal(tr.gflat, first)
    tr.gflat.zero_()
    _lib.check(forward(opts), "matcha_forward")
    _lib.check(backward(), "matcha_backward")
    torch.cuda.synchronize()
    assert torch.equal(tr.gflat, first)                  # deterministic table gradient, dropout seed untouched: the same step again


def test_more_pending_forwards_than_the_record_holds():
    """4 100 pending one-row forwards (the record keeps the 4 096 most recent workspaces), then backward on the newest -- correct -- and on
    the oldest: correct, or the clean "no matcha_forward on record" error; never a result that differs from the twin's."""
    n = 4100
    cfg = C_CFG
    probe = _build(cfg)
    one = probe._runtime().workspace(1, 2).numel()
    if n * one > 3 << 30:
        cfg = replace(CONFIGS["t16"], deterministic=False)
        one = _build(cfg)._runtime().workspace(1, 2).numel()
    del probe
    assert n * one <= 3 << 30, (n, one)
    clf = _build(cfg)
    clf.check_ids = False
    st = S.model_state(clf)
    x = torch.tensor([[3, 17]], device="cuda")
    wt = torch.full((1,), 1.5, device="cuda")
    pending = [_pending_forward(clf, x, wt) for _ in range(n)]
    clf.check_status()
    newest = _grads_of(clf, *pending[-1])
    S.assert_twin("newest pending forward", newest, _twin_autograd(cfg, st, st["seed_counter"] + n - 1, x, wt), cfg)
    e_new = _oracle_autograd("newest pending forward", cfg, clf, st, st["seed_counter"] + n - 1, x, wt, newest)
    try:
        oldest = _grads_of(clf, *pending[0])
    except _lib.MatchaHipError as e:
        assert "no matcha_forward on record" in str(e), e
        verdict = "refused (evicted from the record)"
    else:
        S.assert_twin("oldest pending forward", oldest, _twin_autograd(cfg, st, st["seed_counter"], x, wt), cfg)
        verdict = "correct"
    print(f"{n} pending forwards of {one} workspace bytes each ({cfg.mode} d = {cfg.d}): newest backward bitwise its twin (oracle {e_new:.1e}), oldest {verdict}")
