"""matcha_backward follows the route its forward recorded (model.hip: StepRoute in g_fwd_state) and reads no option.

Through the C ABI, as tests/test_hip_state.py::test_backward_refused_after_forward_only_and_after_a_consumed_forward: a Trainer's buffers,
matcha_forward with targets and loss_in_forward on, matcha_backward, the workspace filled with 0xFF bytes before every forward, a
deterministic Trainer without dropout.  Each flip case runs the forward under one setting of a process-wide switch and the backward under
another; the backward must then launch the kernels of the UN-FLIPPED run of the forward's setting, give its gradients bitwise, and hold the
fp64 oracle's grade (tests/fp64_grade.py, K = 8).  The switches are the ones matcha_backward used to re-read: disable_small_batch (which tail
reduction sums the forward's slabs), disable_fused = 2 (fused front end / fused adj kernels) and disable_fused = 1 after a forward that ran
the tail's backward inside its kernel.  Two sizes: 1 024 rows (small-batch kernels) and the first doubling of it that leaves them.

Bitwise: every gradient on the table front end (deterministic table gradient); on the adj front end every gradient behind the front end --
the adj kernels add their weight gradients with float atomics whatever the Trainer asks (state_twin.Config.bitwise_tensor), so those of
state_twin.FRONT are held to the oracle's grade alone.

A backward whose loss_in_forward / targets do not match what the forward did is refused with MATCHA_EINVAL before any launch.  GPU only (-m gpu).
"""
import ctypes as C

import pytest
import torch

from matcha_amd import _lib
from tests import fp64_grade as G
from tests import state_twin as S
from tests.test_hip_state import _build, _trainer

pytestmark = pytest.mark.gpu

CONFIGS = {"table": S.Config("table", 64, "hg38_1mb", 211), "adj": S.Config("adj", 64, "c23", 213)}
DEFAULT = ("", 0)
_CTX, _PLAIN = {}, {}


class _Ctx:
    """One model + Trainer + batch + oracle references per (front end, size), shared by every case."""

    def __init__(self, mode, size):
        self.cfg = cfg = CONFIGS[mode]
        self.clf = _build(cfg)
        S.set_dropout(self.clf, 0.0)
        self.st = S.model_state(self.clf)
        self.tr = tr = _trainer(self.clf, cfg)
        self.label = f"{mode} {size}"
        rows_per_k = 256                                   # k = 2..5: 1 024 rows, the small-batch kernels
        while True:
            self.batch = S.dev_batch(*G.make_case_batch(cfg.layout, [2, 3, 4, 5], rows_per_k, 531))
            self.B, self.L = self.batch[0].shape
            self.ws, self.logits = tr._buffers(self.B, self.L)
            self.opts = tr._opts(1.0, 0.001, 0)
            with _lib.launch_log() as log:
                _lib.check(self.forward(), "matcha_forward")
                _lib.check(self.backward(), "matcha_backward")
            ran = S.ran_kernels(log)
            assert ("fused_fwd32h_kernel" in ran) != ("fused_fwd32_kernel" in ran), sorted(ran)
            if size == "small" or "fused_fwd32_kernel" in ran:
                break
            rows_per_k *= 2                                # grown until the forward leaves the small-batch kernel
            assert rows_per_k <= 4096, rows_per_k
        assert ("fused_fwd32h_kernel" in ran) == (size == "small"), (size, self.B, sorted(ran))
        x, y, w = (t.cpu().numpy() for t in self.batch)
        self.ref = G.references(S.sd_numpy(self.st), S.oracle_front_end(cfg, self.st), x, y, w, alpha=1.0, beta=0.001, chrom=0)

    def forward(self, opts=None, targets=True):
        tr, rt, (xd, yd, wd) = self.tr, self.tr.rt, self.batch
        self.ws.fill_(0xFF)
        return tr.lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts or self.opts), _lib.ptr(xd), self.B, self.L,
                                     _lib.ptr(yd) if targets else None, _lib.ptr(wd) if targets else None, _lib.ptr(self.logits), _lib.ptr(tr.losses),
                                     _lib.ptr(self.ws), self.ws.numel(), rt.stream())

    def backward(self, opts=None):
        tr, rt, (xd, yd, wd) = self.tr, self.tr.rt, self.batch
        tr.gflat.zero_()
        return tr.lib.matcha_backward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts or self.opts), _lib.ptr(xd), self.B, self.L,
                                      _lib.ptr(yd), _lib.ptr(wd), None, None, C.byref(tr.grads), _lib.ptr(tr.touched), _lib.ptr(self.ws), self.ws.numel(),
                                      rt.stream())

    def step(self, fwd, bwd):
        """Forward under switch ``fwd`` = (name, value), backward under ``bwd``.  Returns (outputs, kernels of the backward call)."""
        with _lib.option(*fwd) if fwd[0] else S.option(""):
            _lib.check(self.forward(), "matcha_forward")
        with (_lib.option(*bwd) if bwd[0] else S.option("")), _lib.launch_log() as log:
            _lib.check(self.backward(), "matcha_backward")
        torch.cuda.synchronize()
        got = {"logits": self.logits.clone(), "losses": self.tr.losses.clone()}
        got.update({"grad/" + n: g for n, g in S.trainer_grads(self.tr, self.clf).items()})
        return got, S.ran_kernels(log)

    def graded(self, label, got):
        ls = got["losses"].cpu().numpy()
        grads = {n: None for n in self.ref.r64.grads}
        grads.update({k[5:]: (None if v is None else v.cpu().double().numpy()) for k, v in got.items() if k.startswith("grad/")})
        G.assert_grade(label, G.grade(G.StepOut(got["logits"].cpu().double().numpy(), {"bce": float(ls[0]), "recon": float(ls[1])}, grads), self.ref))

    def bitwise(self, name):
        return self.cfg.mode == "table" or not name.startswith(S.FRONT)


def _ctx(mode, size):
    if (mode, size) not in _CTX:
        _CTX[mode, size] = _Ctx(mode, size)
    return _CTX[mode, size]


def _plain(c, setting):
    """The un-flipped run of a setting (forward and backward under it): computed once, itself held to the oracle."""
    key = (c.label, setting)
    if key not in _PLAIN:
        got, ran = c.step(setting, setting)
        c.graded(f"{c.label}, {setting}", got)
        _PLAIN[key] = (got, ran)
    return _PLAIN[key]


SMALL_OFF, FRONT_OFF, FUSED_OFF = ("disable_small_batch", 1), ("disable_fused", 2), ("disable_fused", 1)
FLIPS = [("table", "small", DEFAULT, SMALL_OFF), ("table", "small", SMALL_OFF, DEFAULT)]                     # (a)
FLIPS += [(m, s, f, b) for m in ("table", "adj") for s in ("small", "large") for f, b in ((DEFAULT, FRONT_OFF), (FRONT_OFF, DEFAULT))]      # (b)
FLIPS += [("table", s, DEFAULT, FUSED_OFF) for s in ("small", "large")]                                      # (c)


@pytest.mark.parametrize("mode,size,fwd,bwd", FLIPS, ids=lambda v: v if isinstance(v, str) else f"{v[0] or 'default'}={v[1]}")
def test_backward_follows_the_recorded_route(mode, size, fwd, bwd):
    c = _ctx(mode, size)
    want, want_ran = _plain(c, fwd)
    got, ran = c.step(fwd, bwd)
    label = f"{c.label}: forward {fwd}, backward {bwd}"
    assert ran == want_ran, (label, "only flipped", sorted(ran - want_ran), "only un-flipped", sorted(want_ran - ran))
    if fwd == DEFAULT:
        assert "head_bwd_kernel" not in ran and "fused_bwdh_kernel" in ran, sorted(ran)       # the tail's backward ran in the forward: the fused record
    assert set(got) == set(want)
    front_same = 0
    for k, v in want.items():
        if v is None:
            assert got[k] is None, (label, k)
        elif not k.startswith("grad/") or c.bitwise(k[5:]):
            assert torch.equal(got[k], v), (label, k, float((got[k] - v).abs().max()))
        else:
            front_same += int(torch.equal(got[k], v))
    print(f"{label}: backward ran {len(ran)} kernels as the un-flipped run; bitwise everywhere asserted, {front_same} front-end tensors bitwise too")
    c.graded(label, got)


def _refused(c, call):
    with _lib.launch_log() as log:
        rc = call()
    msg = c.tr.lib.matcha_last_error().decode()
    assert rc == -22 and "loss_in_forward / targets differ from the forward's on this workspace" in msg, (rc, msg)      # MATCHA_EINVAL
    assert not S.ran_kernels(log), sorted(S.ran_kernels(log))                                                           # refused before any launch


def test_backward_refuses_another_loss_in_forward_than_the_forwards():
    c = _ctx("table", "small")
    want, _ = _plain(c, DEFAULT)
    off = c.tr._opts(1.0, 0.001, 0)
    off.loss_in_forward = 0
    _lib.check(c.forward(), "matcha_forward")                      # the tail's backward ran in the forward kernel ...
    _refused(c, lambda: c.backward(off))                           # ... and this backward would run head_bwd over the parked rows
    _lib.check(c.forward(targets=False), "matcha_forward")         # no targets: no loss, nothing of the tail's backward ...
    _refused(c, c.backward)                                        # ... which this backward takes for done
    got, _ = c.step(DEFAULT, DEFAULT)                              # a fresh forward makes the workspace usable again
    for k, v in want.items():
        assert (got[k] is None and v is None) or torch.equal(got[k], v), k
