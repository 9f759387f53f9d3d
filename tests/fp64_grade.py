"""fp32 grade: one accuracy criterion for every output of a training step, against the fp64 oracle.

The north-star tolerance (1e-4 relative) sits more than 100x above what fp32 arithmetic achieves here (~3e-7 on logits), so a kernel
could lose a factor of 20 in precision -- drop a bf16 plane product, say -- and still pass every parity test.  This module holds the
HIP path (or any candidate) to the noise of fp32 itself:

* ``R64``  the oracle in fp64 on the fp32 inputs: the exact answer, up to rounding;
* ``R32a`` the oracle in fp32;
* ``R32b`` the oracle in fp32 on the row-permuted batch, outputs un-permuted: a second sample of legitimate reordering noise (it only
  differs from R32a in reductions over rows, i.e. in the gradients).

For an output X, ``e(X) = max|X - R64| / max|R64|`` per tensor (and for the logits also the element-wise ``logit_err``); the check is
``e(X) <= K * max(e(R32a), e(R32b), 2^-23)`` with K = 8.  The gauge tensor (true gradient 0) stays excluded.

Two witnesses show that the criterion has power (tests/test_cpu_fp64_oracle.py): ``THREE_PRODUCT`` replaces every matrix product of
the oracle by the three bf16 plane products Ah Bh + Ah Bm + Am Bh (the six-product scheme of the fused kernels with the low planes
dropped), ``FAST_TANH`` replaces tanh by the one-exp formula (e^{2x} - 1) / (e^{2x} + 1) evaluated in f32, which
matcha_amd/csrc/common.hpp's fast_tanh used for every x before it got its small-|x| polynomial.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from matcha_amd import synth
from oracle import hypersagnn as O
from oracle import rng as R
from tests.helpers import logit_err

K = 8.0
ULP = 2.0 ** -23
GAUGE = "encode1.mul_head_attn.layer_norm2.bias"     # true gradient 0 (tests/test_oracle_golden.py)
FROZEN = "attribute_dict_embedding.weight"          # frozen attribute table (Modules.py:247); the model also names it attribute_dict.weight
FROZEN_NAMES = {FROZEN, "attribute_dict.weight"}


# --------------------------------------------------------------------------------------------------------------------------------
# witnesses: reduced-precision arithmetic the criterion must reject
# --------------------------------------------------------------------------------------------------------------------------------
def _planes(a):
    """(h, m): the two high bf16 planes of an f32 tensor (round to nearest even, like v_cvt_pk_bf16_f32), returned as f32."""
    h = a.to(torch.bfloat16).to(torch.float32)
    return h, (a - h).to(torch.bfloat16).to(torch.float32)


def _mm3(a, b):
    """a @ b as the three plane products Ah Bh + Ah Bm + Am Bh: exact bf16 x bf16 products, f32 accumulation."""
    ah, am = _planes(a.to(torch.float32))
    bh, bm = _planes(b.to(torch.float32))
    return torch.matmul(ah, bh) + (torch.matmul(ah, bm) + torch.matmul(am, bh))


class _ThreeProduct(torch.autograd.Function):
    """a @ b (2-D or batched 3-D) with the backward's two products in the same three-product scheme."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _mm3(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = _mm3(g, b.transpose(-1, -2)) if ctx.needs_input_grad[0] else None
        gb = _mm3(a.transpose(-1, -2), g) if ctx.needs_input_grad[1] else None
        return ga, gb


def three_product_mm(a, b):
    if a.dim() > 2 and b.dim() == 2:          # activations [B, L, d] times a weight: one 2-D product over the flattened rows
        return _ThreeProduct.apply(a.reshape(-1, a.shape[-1]), b).view(*a.shape[:-1], b.shape[-1])
    return _ThreeProduct.apply(a, b)


class _FastTanh(torch.autograd.Function):
    """(e^{2x} - 1) / (e^{2x} + 1) in f32 with x clamped to +-15 (~1e-7 absolute error at every x); backward 1 - y^2."""

    @staticmethod
    def forward(ctx, x):
        xc = x.to(torch.float32).clamp(-15.0, 15.0)
        e = torch.exp(2.0 * xc)
        y = (e - 1.0) / (e + 1.0)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * (1.0 - y * y)


THREE_PRODUCT = O.Ops(mm=three_product_mm, bmm=three_product_mm)
FAST_TANH = O.Ops(tanh=_FastTanh.apply)


# --------------------------------------------------------------------------------------------------------------------------------
# the references
# --------------------------------------------------------------------------------------------------------------------------------
@dataclass
class StepOut:
    """What one training step produces, as float64 numpy: logits [B], the losses by name, the gradients (None = not reached)."""
    logits: np.ndarray
    losses: Dict[str, float]
    grads: Dict[str, Optional[np.ndarray]]


def main_loss_name(objective):
    return "mse" if objective == "regress" else "bce"


def oracle_step(sd, fe, x, y, w, *, alpha=1.0, beta=0.001, chrom=0, dtype=torch.float32, perm=None, ops=O.TORCH_OPS,
                objective="class", backward=True, masks=None) -> StepOut:
    """One step of the oracle in ``dtype`` on the state dict ``sd`` (numpy, fp32) and the batch x [B, L], y / w [B]:
    loss = objective * alpha + recon * beta (bce: main.py:56; regress: mse of softplus, main.py:60-66).  ``perm`` permutes the batch
    rows before the step; the logits come back in the original order.  ``masks`` (None: dropout-free) are the float32 multiplier masks of
    ``step_masks``, rows in token-slot order b L + l: they are inputs like the weights -- the f32 value 1 / (1 - p) is cast to ``dtype``, exact
    in fp64 -- and are permuted with their rows."""
    P = {k: torch.from_numpy(np.array(v)).to(dtype).requires_grad_(backward and k not in FROZEN_NAMES) for k, v in sd.items()}
    fe = fe.to(dtype)
    x, y = torch.as_tensor(x), torch.as_tensor(y).reshape(-1, 1).to(dtype)
    w = None if w is None else torch.as_tensor(w).reshape(-1, 1).to(dtype)
    if perm is not None:
        p = torch.as_tensor(perm)
        x, y, w = x[p], y[p], (None if w is None else w[p])
    if masks is not None:
        B, L = x.shape
        masks = {k: torch.from_numpy(np.asarray(m, dtype=np.float32)).to(dtype).view(B, L, -1) for k, m in masks.items()}
        masks = {k: (m if perm is None else m[p]).reshape(B * L, -1) for k, m in masks.items()}
    with torch.set_grad_enabled(backward):
        logits, recon = O.classifier_forward(P, fe, x, random_chrom=chrom, ops=ops, masks=masks)
        if objective == "regress":
            main = F.mse_loss(F.softplus(logits), y)
        else:
            main = O.bce_with_logits(logits, y, w)
        grads = {}
        if backward:
            names = [n for n, t in P.items() if t.requires_grad]
            gs = torch.autograd.grad(main * alpha + recon * beta, [P[n] for n in names], allow_unused=True)
            grads = {n: (None if g is None else g.detach().double().numpy()) for n, g in zip(names, gs)}
    lg = logits.detach().double().numpy().reshape(-1)
    if perm is not None:
        back = np.empty_like(lg)
        back[np.asarray(perm)] = lg
        lg = back
    return StepOut(lg, {main_loss_name(objective): float(main.detach()), "recon": float(recon.detach().reshape(-1)[0])}, grads)


def step_masks(seed, ps, n_tokens, d, num=None, wrap=None):
    """The multiplier masks {"fc1", "pff"[, "adj"]: float32 [n_tokens, d | max(num)]} of a step with dropout seed ``seed`` and
    ps = (p_adj, p_fc1, p_pff) (Classifier._dropout_p()), as the kernels draw them (oracle/rng.py): the counter's high word is the token slot
    b L + l over all B L slots, padding included.  ``num`` is the layout on the adj front end, None on the table front end.  ``wrap`` is
    applied to each mask (tests/state_twin.py::call_masks: torch.from_numpy).  A Trainer(clf, base_seed=S) draws its first step with S + 1."""
    p_adj, p_fc1, p_pff = ps
    masks = {"fc1": R.dropout_mask(seed, R.STREAM_DROP_FC1, p_fc1, n_tokens, d),
             "pff": R.dropout_mask(seed, R.STREAM_DROP_PFF, p_pff, n_tokens, d)}
    if num is not None:
        masks["adj"] = R.dropout_mask(seed, R.STREAM_DROP_ADJ, p_adj, n_tokens, int(max(num)))
    return {k: wrap(m) for k, m in masks.items()} if wrap else masks


@dataclass
class References:
    r64: StepOut
    r32a: StepOut
    r32b: StepOut


def references(sd, fe, x, y, w, *, perm_seed=0, **kw) -> References:
    """R64, R32a and R32b of one step (module docstring); ``masks=`` of oracle_step goes to all three."""
    perm = np.random.default_rng(perm_seed).permutation(len(x))
    return References(oracle_step(sd, fe, x, y, w, dtype=torch.float64, **kw), oracle_step(sd, fe, x, y, w, **kw),
                      oracle_step(sd, fe, x, y, w, perm=perm, **kw))


# --------------------------------------------------------------------------------------------------------------------------------
# the criterion
# --------------------------------------------------------------------------------------------------------------------------------
def tensor_err(a, r):
    """max|a - r| / max|r| (absolute where r is 0 everywhere)."""
    a = np.asarray(a, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    den = float(np.abs(r).max()) if r.size else 0.0
    return float(np.abs(a - r).max()) / (den if den > 0 else 1.0)


@dataclass
class Row:
    what: str
    err: float
    noise: float
    k: float

    @property
    def ratio(self):
        return self.err / self.noise

    @property
    def ok(self):
        return self.err <= self.k * self.noise


def row(what, got, r64, r32a, r32b, k=K, err=tensor_err):
    """One row of the criterion: e(got) against max(e(R32a), e(R32b), 2^-23), all against R64."""
    noise = max(err(r32a, r64), err(r32b, r64), ULP)
    return Row(what, err(got, r64), noise, k)


def logit_rows(logits, ref: References, k=K):
    """The two logit checks: norm-wise e and the element-wise logit_err, both against R64."""
    lg = np.asarray(logits, dtype=np.float64).reshape(-1)
    refs = (ref.r64.logits, ref.r32a.logits, ref.r32b.logits)
    return [row("logits", lg, *refs, k), row("logits (element-wise)", lg, *refs, k, err=logit_err)]


def grade(got: StepOut, ref: References, k_of: Optional[Dict[str, float]] = None, skip=(GAUGE,), k_max=16.0):
    """Every row of the criterion for one step: logits (both ways), the losses, every gradient tensor but ``skip``.  ``k_of`` maps a
    tensor name to a larger K (at most ``k_max``, with its reason where it is set).  Asserts that the grad-None sets are equal."""
    k_of = k_of or {}
    assert max(k_of.values(), default=K) <= k_max
    none_got = {n for n, v in got.grads.items() if v is None and n not in FROZEN_NAMES}
    none_ref = {n for n, v in ref.r64.grads.items() if v is None and n not in FROZEN_NAMES}
    assert none_got == none_ref, ("grad-None sets differ", sorted(none_got ^ none_ref))
    rows = logit_rows(got.logits, ref, k_of.get("logits", K))
    for name, v in got.losses.items():
        refs = (np.array([s.losses[name]]) for s in (ref.r64, ref.r32a, ref.r32b))
        rows.append(row(name, np.array([v]), *refs, k_of.get(name, K)))
    for name, g64 in ref.r64.grads.items():
        if g64 is None or name in skip:
            continue
        rows.append(row(name, got.grads[name], g64, ref.r32a.grads[name], ref.r32b.grads[name], k_of.get(name, K)))
    return rows


def assert_grade(label, rows):
    """Print the worst ratio e / noise of a case and fail on every row above its K."""
    worst = max(rows, key=lambda r: r.ratio)
    print(f"{label}: worst e/noise {worst.ratio:5.2f} ({worst.what}: e {worst.err:.2e}, noise {worst.noise:.2e}) over {len(rows)} outputs")
    bad = [(r.what, f"e {r.err:.2e}", f"noise {r.noise:.2e}", f"ratio {r.ratio:.1f} > K {r.k:g}") for r in rows if not r.ok]
    assert not bad, (label, bad)
    return worst.ratio


# --------------------------------------------------------------------------------------------------------------------------------
# stress transforms of a synth.make_state_dict state dict (applied before it is loaded into the model and the oracle)
# --------------------------------------------------------------------------------------------------------------------------------
def small_amplitude(sd):
    """next_w (and on the adj front end every tied weight_0) x 0.02: the tanh arguments shrink to |x| <~ 0.05."""
    out = dict(sd)
    for k in ("next_w.FF_Linear0.weight", "next_w.FF_Linear0.bias"):
        out[k] = (np.asarray(sd[k]) * np.float32(0.02)).astype(np.float32)
    for k in sd:
        if k.endswith("tied weight_0"):
            out[k] = (np.asarray(sd[k]) * np.float32(0.02)).astype(np.float32)
    return out


def sharp_attention(sd):
    """w_qs and w_ks x 6: scores of about +-60 (max subtraction, the closed-form pad key)."""
    out = dict(sd)
    for k in ("encode1.mul_head_attn.w_qs.weight", "encode1.mul_head_attn.w_ks.weight"):
        out[k] = (np.asarray(sd[k]) * np.float32(6.0)).astype(np.float32)
    return out


def saturated_logits(sd, fe, x, chrom=0, target=40.0):
    """pff_classifier's weight and bias scaled so that max |logit| over the batch is ``target``."""
    with torch.no_grad():
        P = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
        lg, _ = O.classifier_forward(P, fe, torch.as_tensor(x), random_chrom=chrom)
    s = np.float32(target / float(lg.abs().max()))
    out = dict(sd)
    for k in ("pff_classifier.PWF_Conv0.weight", "pff_classifier.PWF_Conv0.bias"):
        out[k] = (np.asarray(sd[k]) * s).astype(np.float32)
    return out


def saturated_pff(sd, fe, x, chrom=0, target=4.0):
    """encode1.pff_n1's first layer (weight and bias) scaled so that the 99th percentile of |pre-activation| over the batch's real tokens is
    ``target``: at 4, tanh' = 1 - t^2 ~ 1e-3, where a backward that recovers t from a stored t / (1 - p) as (t / (1 - p)) (1 - p) loses the
    most.  The scale is taken from the dropout-free forward."""
    pp = "encode1.pff_n1.PWF_Conv0."
    with torch.no_grad():
        P = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
        xt = torch.as_tensor(x)
        _, _, mid = O.classifier_forward(P, fe, xt, random_chrom=chrom, return_intermediates=True)
        pre = mid["y"] @ P[pp + "weight"][:, :, 0].t() + P[pp + "bias"]
        q = float(np.quantile(pre[xt != 0].abs().numpy().astype(np.float64), 0.99))
    s = np.float32(target / q)
    out = dict(sd)
    for k in (pp + "weight", pp + "bias"):
        out[k] = (np.asarray(sd[k]) * s).astype(np.float32)
    return out


def hot_node(x, frac, node=1):
    """Node ``node`` put into the first slot of a fraction ``frac`` of the rows (rows stay ascending and duplicate-free)."""
    x = np.array(x, copy=True)
    rows = np.flatnonzero((x[:, 1] > node) & (x[:, 0] != node))
    x[rows[: int(np.ceil(frac * len(x)))], 0] = node
    return x


def make_case_batch(layout, ks, rows_per_k, seed, L=0):
    """(x int64 [B, L], y float32 [B], w float32 [B]) of synth.make_batch."""
    x, y, w = synth.make_batch(np.random.default_rng(seed), int(np.sum(synth.LAYOUTS[layout])), ks, rows_per_k, L)
    return x, y.reshape(-1), w.reshape(-1)


def halves_cap(T, L):
    """ragged.hip halves_cap: the half tiles the ragged plan provisions for T tokens of rows of L slots."""
    cdiv = lambda a, b: -(-a // b)
    return cdiv(T + 1, 32 - L) + cdiv(T + 1, 63 * 32)


def edge_rows(which, L):
    """The batch size at which halves_cap(B L, L) last stays at 2 CU (edge-: the small-batch forward) and the next one (edge+)."""
    cap = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    B = 1
    while halves_cap((B + 1) * L, L) <= cap:
        B += 1
    assert halves_cap(B * L, L) <= cap < halves_cap((B + 1) * L, L)
    return B if which == "edge-" else B + 1
