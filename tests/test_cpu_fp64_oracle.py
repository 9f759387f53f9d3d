"""The fp32-grade criterion of tests/fp64_grade.py, checked for power on the CPU before any GPU result leans on it.

(a) At three shapes, a third legitimate fp32 summation order (the oracle on another row permutation) passes the criterion, and the
    three-product witness -- every product as Ah Bh + Ah Bm + Am Bh, its backward too -- fails it by at least 2x on the logits and on
    the gradients of the products it replaces.  The fast_tanh witness fails it on a small-amplitude model.  The same with dropout ON
    (masks injected into every reference), plus: all-ones masks change nothing, a wrong mask is rejected.
(b) The oracle's formulation is pinned at fp32 grade, not just at the 2e-5 of tests/test_oracle_golden.py: every reference fixture's
    fp32 output (in the role the HIP path plays on the GPU) meets the criterion against the fp64 oracle.  CPU only.
"""
import numpy as np
import pytest
import torch

from matcha_amd import synth
from tests import fp64_grade as G
from tests.helpers import G3BIG, g3big_batch, g3big_grad_ref, gold, oracle_state
from tests.test_cpu_regress import GR, gr_ref
from tests.test_oracle_golden import CASES as G2_CASES

# the gradients of the products the witness replaces (the logits are checked two ways; they fail if either way does)
WITNESS_TARGETS = ["encode1.mul_head_attn.w_qs.weight", "encode1.mul_head_attn.w_ks.weight", "encode1.mul_head_attn.w_vs.weight",
                   "encode1.mul_head_attn.fc1.weight", "next_w.FF_Linear0.weight"]

# name -> (layout, embed_dim, front end, weight seed, ks, rows per k)
POWER = {"hg38_table_d64": ("hg38_1mb", 64, "table", 121, (2, 3, 4, 5), 500),
         "c1_table_d128": ("c1", 128, "table", 122, (2, 3, 4, 5, 6, 7, 8), 286),
         "wide_adj_d64": ("wide_adj", 64, "adj", 113, (2, 3, 4, 5), 500)}


def _power_case(name):
    layout, d, mode, seed, ks, rows = POWER[name]
    _, fe, sd = oracle_state(synth.LAYOUTS[layout], d, mode, seed)
    x, y, w = G.make_case_batch(layout, list(ks), rows, seed + 500)
    return sd, fe, x, y, w, seed % fe.n_chrom


def _power_masks(name, x, ps, seed=77):
    """The masks of a step on POWER[name]'s batch ``x`` with ps = (p_adj, p_fc1, p_pff) and dropout seed ``seed``."""
    layout, d, mode = POWER[name][:3]
    return G.step_masks(seed, ps, x.size, d, synth.LAYOUTS[layout] if mode == "adj" else None)


def _assert_power(label, sd, fe, x, y, w, chrom, masks=None):
    """A third row order of the fp32 oracle passes the criterion, the three-product witness is >= 2x over its bound on the logits and on
    every one of WITNESS_TARGETS; returns the references."""
    ref = G.references(sd, fe, x, y, w, chrom=chrom, masks=masks)
    third = G.oracle_step(sd, fe, x, y, w, chrom=chrom, perm=np.random.default_rng(1).permutation(len(x)), masks=masks)
    G.assert_grade(f"{label} fp32, third row order", G.grade(third, ref))
    rows = {r.what: r for r in G.grade(G.oracle_step(sd, fe, x, y, w, chrom=chrom, ops=G.THREE_PRODUCT, masks=masks), ref)}
    over = {t: rows[t].err / (rows[t].k * rows[t].noise) for t in ["logits", "logits (element-wise)"] + WITNESS_TARGETS}
    over["logits"] = max(over.pop("logits"), over.pop("logits (element-wise)"))
    print(f"{label}: three-product witness, e / bound: " + ", ".join(f"{t.split('.')[-2] if '.' in t else t} {v:.1f}" for t, v in over.items()))
    assert min(over.values()) >= 2.0, over
    return ref


@pytest.mark.parametrize("name", sorted(POWER))
def test_reordered_fp32_passes_and_the_three_product_witness_fails(name):
    _assert_power(name, *_power_case(name))


# The criterion under dropout: the masks are inputs of the step (float32 multipliers 0 or 1 / (1 - p), exact in fp64), so the noise floor and
# the witness's margin must survive them -- at the model's default p and at p no float represents, where nine tenths of pff_n1's hidden
# layer is dropped and the rest scaled by 10.
P_DEFAULT, P_HIGH = (0.2, 0.3, 0.4), (0.6, 0.7, 0.9)


@pytest.mark.parametrize("name,ps", [(n, P_DEFAULT) for n in sorted(POWER)] + [("hg38_table_d64", P_HIGH)])
def test_criterion_has_power_with_dropout_on(name, ps):
    sd, fe, x, y, w, chrom = _power_case(name)
    _assert_power(f"{name} p {ps}", sd, fe, x, y, w, chrom, masks=_power_masks(name, x, ps))


@pytest.mark.parametrize("name", ["hg38_table_d64", "wide_adj_d64"])
def test_masks_reach_every_reference(name):
    """All-ones masks (every p = 0) are the mask-free step bit for bit, in every reference; and a candidate that differs from the references
    in ONE mask only (another seed's) fails the criterion, whichever mask it is -- a reference that dropped a mask, or left it in place
    under the row permutation, would make the three disagree or the candidate pass."""
    sd, fe, x, y, w, chrom = _power_case(name)
    plain = G.references(sd, fe, x, y, w, chrom=chrom)
    ones = G.references(sd, fe, x, y, w, chrom=chrom, masks=_power_masks(name, x, (0.0, 0.0, 0.0)))
    for a, b in zip((plain.r64, plain.r32a, plain.r32b), (ones.r64, ones.r32a, ones.r32b)):
        assert np.array_equal(a.logits, b.logits) and a.losses == b.losses and a.grads.keys() == b.grads.keys()
        assert all((a.grads[n] is None and b.grads[n] is None) or np.array_equal(a.grads[n], b.grads[n]) for n in a.grads)
    masks, other = _power_masks(name, x, P_DEFAULT), _power_masks(name, x, P_DEFAULT, seed=78)
    ref = G.references(sd, fe, x, y, w, chrom=chrom, masks=masks)
    G.assert_grade(f"{name} own masks", G.grade(G.oracle_step(sd, fe, x, y, w, chrom=chrom, masks=masks), ref))
    for key in masks:
        rows = G.grade(G.oracle_step(sd, fe, x, y, w, chrom=chrom, masks={**masks, key: other[key]}), ref)
        worst = max(rows, key=lambda r: r.ratio)
        print(f"{name}: {key} mask of another seed, worst e / bound {worst.err / (worst.k * worst.noise):.3g} ({worst.what})")
        assert worst.err >= 100.0 * worst.k * worst.noise, (key, worst.what, worst.ratio)


def test_fast_tanh_witness_fails_at_small_amplitude():
    """tanh through one exp is accurate to ~1e-7 absolute, so its relative error grows as 1 / |x|: with next_w x 0.02 every
    tanh(next_w ...) argument is below ~0.05 and the criterion must notice the difference."""
    sd, fe, x, y, w, chrom = _power_case("hg38_table_d64")
    sd = G.small_amplitude(sd)
    ref = G.references(sd, fe, x, y, w, chrom=chrom)
    rows = G.grade(G.oracle_step(sd, fe, x, y, w, chrom=chrom, ops=G.FAST_TANH), ref)
    worst = max(rows, key=lambda r: r.ratio)
    print(f"fast_tanh witness at small amplitude: worst {worst.what} e / bound {worst.err / (worst.k * worst.noise):.1f}")
    assert worst.err >= 2.0 * worst.k * worst.noise, (worst.what, worst.ratio)


# ---- (b) the reference's own fp32 outputs against the fp64 oracle ---------------------------------------------------------------------
# The biases of the reference's Conv1d(k = 1) layers (pff_n1 Modules.py:357-362, pff_classifier :299) get their gradient from the conv
# backward: one f32 reduction over all B L tokens in the convolution's own order, where the oracle (and the HIP path) sum as a Linear
# does.  With tens of thousands of cancelling addends that reduction is measured at up to 32x the oracle's fp32 noise (g3big / gr at
# 9 216 rows; 10x for pff_classifier) -- the reference's arithmetic, not the oracle's formulation: the same three tensors of the HIP path
# stay within K = 8 on every case of tests/test_hip_fp64_grade.py.  They are held to 40x here; every other output to K = 8.
CONV1D_BIAS = {"encode1.pff_n1.PWF_Conv0.bias": 40.0, "encode1.pff_n1.PWF_Conv1.bias": 40.0, "pff_classifier.PWF_Conv0.bias": 40.0}

def _strided(out: G.StepOut, stride_of):
    """The gradients of ``out`` at the stored elements of a fixture (every stride-th element of the flattened tensor)."""
    return G.StepOut(out.logits, out.losses, {n: (None if v is None else v.reshape(-1)[::stride_of[n]]) for n, v in out.grads.items()})


def _grade_fixture(label, g, sd, fe, x, y, w, chrom, cand_logits, cand_losses, grad_ref, alpha=1.0, beta=0.001, objective="class"):
    ref = G.references(sd, fe, x, y, w, chrom=chrom, alpha=alpha, beta=beta, objective=objective)
    none_ref = set(g["grad_none"].tolist()) - G.FROZEN_NAMES
    grads, strides = {}, {}
    for n, v in ref.r64.grads.items():
        if v is None:
            grads[n] = None
            continue
        strides[n], grads[n] = grad_ref(n)
    assert {n for n, v in grads.items() if v is None} == none_ref
    for n in strides:
        if strides[n] is None:             # not stored in the fixture: compare the oracle with itself (ratio 0), it is checked elsewhere
            strides[n], grads[n] = 1, ref.r64.grads[n].reshape(-1)
    ref = G.References(*(_strided(r, strides) for r in (ref.r64, ref.r32a, ref.r32b)))
    cand = G.StepOut(np.asarray(cand_logits, dtype=np.float64).reshape(-1), cand_losses, grads)
    G.assert_grade(label, G.grade(cand, ref, CONV1D_BIAS, k_max=40.0))


@pytest.mark.parametrize("name,layout,d,mode,seed", G2_CASES)
def test_g2_reference_logits_at_fp32_grade(name, layout, d, mode, seed):
    g = gold(f"g2_{name}.npz")
    _, fe, sd = oracle_state(synth.LAYOUTS[layout], d, mode, seed)
    for key in ("k2", "k3", "k4", "k5", "mixed"):
        x = g[f"x_{key}"]
        chrom = int(g[f"chrom_{key}"])
        outs = [G.oracle_step(sd, fe, x, np.zeros(len(x), np.float32), np.ones(len(x), np.float32), chrom=chrom, dtype=dt, perm=p,
                              backward=False)
                for dt, p in ((torch.float64, None), (torch.float32, None), (torch.float32, np.random.default_rng(0).permutation(len(x))))]
        rows = G.logit_rows(g[f"logits_{key}"], G.References(*outs))
        if mode == "adj":
            rows.append(G.row("recon", g[f"recon_{key}"], *(np.array([o.losses["recon"]]) for o in outs)))
        G.assert_grade(f"g2 {name} {key}", rows)


@pytest.mark.parametrize("name,mode,seed", [("hg38_table_d64", "table", 46), ("hg38_adj_d64", "adj", 47)])
def test_g3g_reference_step_at_fp32_grade(name, mode, seed):
    g = gold(f"g3g_{name}.npz")
    _, fe, sd = oracle_state(synth.LAYOUTS["hg38_1mb"], 64, mode, seed)

    def grad_ref(n):
        if ("grad0/" + n) in g.files:
            return 1, g["grad0/" + n].reshape(-1)
        return 8, g["grad0s8/" + n]
    _grade_fixture(f"g3g {name}", g, sd, fe, g["x0"], g["y0"], g["w0"], int(g["chroms"][0]), g["logits0"],
                   {"bce": float(g["bce0"]), "recon": float(g["recon0"][0])}, grad_ref)


@pytest.mark.parametrize("name", sorted(G3BIG))
def test_g3big_reference_step_at_fp32_grade(name):
    layout, d, mode, seed = G3BIG[name]
    g = gold(f"g3big_{name}.npz")
    _, fe, sd = oracle_state(synth.LAYOUTS[layout], d, mode, seed)
    x, y, w = (t.numpy() for t in g3big_batch(g))
    _grade_fixture(f"g3big {name}", g, sd, fe, x, y, w, int(g["chroms"][0]), g["logits0"],
                   {"bce": float(g["bce0"]), "recon": float(g["recon0"][0])}, lambda n: g3big_grad_ref(g, n))


@pytest.mark.parametrize("name", sorted(GR))
def test_gr_reference_regress_step_at_fp32_grade(name):
    layout, d, mode, seed = GR[name]
    g = gold(f"gr_{name}.npz")
    _, fe, sd = oracle_state(synth.LAYOUTS[layout], d, mode, seed)
    _grade_fixture(f"gr {name}", g, sd, fe, g["x0"].astype(np.int64), g["y0"], None, int(g["chroms"][0]), g["logits0"],
                   {"mse": float(g["mse0"]), "recon": float(g["recon0"][0])}, lambda n: gr_ref(g, "grad0", n),
                   alpha=float(g["alpha"][0]), beta=float(g["beta"][0]), objective="regress")
