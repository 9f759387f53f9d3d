"""The long rows (9 to 32 nodes) on the device at every width with every k in one batch, under the stresses of tests/fp64_grade.py, at every
embed_dim check_shape_fields accepts, and the attention backward alone on the whole (L, k) grid: model(x), get_embedding(x) and one training step
against the fp64 oracle at fp32 grade (tests/fp64_grade.py as it is, K = 8), the attention probabilities in closed form where every score is 0,
and matcha_attn_long_bwd against torch fp64 autograd.  The batches and their power test are in tests/test_cpu_long_grid.py.  GPU only (-m gpu)."""
import numpy as np
import pytest
import torch

from matcha_amd import synth
from tests import fp64_grade as G
from tests.helpers import logit_err
from tests.test_cpu_long_embedding import embedding_refs, grade_rows
from tests.test_cpu_long_grid import (BETA, EVERY_K, FOURPROD, HOT_L, HOT_ROWS, KEYS, MERGED, P_DEFAULT, batch_of, key_id,
                                      torch_attention_grads_by_k)
from tests.test_hip_long_embedding import LONG_EMB, NOT_HERE, assert_structure, embed
from tests.test_hip_long_rows import LONG, SHORT_ONLY, model as eval_model, run
from tests.test_hip_long_train import LONG_TRAIN, SHORT_BWD, TOL, attention_backward_case, model as train_model, step
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

# Rows of G.grade that need K above 8 (at most 16), each with its cancellation argument: none so far.
K_OF = {}

RESULTS, BWD_RESULTS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    if RESULTS:
        print("\nlong rows, fp32 grade: worst e(HIP) / noise per batch (forward: model(x) logits; embedding: attn, dynamic, static; step: logits, "
              "losses, every gradient)")
        for name, r in RESULTS.items():
            print(f"  {name:48s} " + "   ".join(f"{what} {r[what]:5.2f}" for what in ("forward", "embedding", "step", "step, dropout") if what in r))
    if BWD_RESULTS:
        print("\nattention backward alone: worst e / torch fp32's error over the cases of a group (dQ, dK, dV; the padding token's dK / dV row alone)")
        for name, r in BWD_RESULTS.items():
            print(f"  {name:28s} " + "   ".join(f"{what} {v:5.2f}" for what, v in r.items()))


# ---- models, references ------------------------------------------------------------------------------------------------------------------------------
_STRESSED, _REFS, _EREFS = {}, {}, {}


def clf_of(key, train, dropout=False):
    """The key's model on the device in eval or train mode: the three long-row test files' own models where the weights are the case's, one
    built on the stressed state dict otherwise (long_row_training on, dropout off unless asked)."""
    case, L, kind, s, _ = key
    if s in ("", "hot"):
        return train_model(*case, dropout=dropout)[0] if train else eval_model(*case)[0]
    ck = (case, L, s, dropout)
    if ck not in _STRESSED:
        clf, _ = hip_model(synth.LAYOUTS[case[0]], case[1], case[2], case[3], sd=batch_of(key)[0])
        if not dropout:
            for m in clf.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
        clf.long_row_training = True
        _STRESSED[ck] = clf
    return _STRESSED[ck].train() if train else _STRESSED[ck].eval()


def refs_of(key):
    """The dropout-free step's References of a key (their logits are model(x)'s as well)."""
    if key not in _REFS:
        sd, fe, x, y, w, chrom = batch_of(key)
        _REFS[key] = G.references(sd, fe, x, y, w, chrom=chrom, beta=BETA)
    return _REFS[key]


def ks_of(x):
    return [int(k) for k in (x != 0).sum(1)]


def graded(key, what, rows, x, lg=None):
    """G.assert_grade with the batch named in the failure: the width, every row's k, and for the logits the row that is worst."""
    label = f"{what} {key_id(key)}"
    try:
        ratio = G.assert_grade(label, rows)
    except AssertionError as e:
        ks = ks_of(x)
        detail = f"L = {x.shape[1]}, rows' k = {ks if len(ks) <= 65 else (min(ks), '..', max(ks))}"
        if lg is not None:
            b = int(np.abs(lg - refs_of(key).r64.logits).argmax())
            detail += f"; worst logit in row {b}, k = {ks[b]}, slots {np.flatnonzero(x[b]).tolist()}"
        raise AssertionError(f"{e} -- {detail}") from None
    RESULTS.setdefault(key_id(key), {})[what] = ratio
    return ratio


def forward_graded(key):
    sd, fe, x, y, w, chrom = batch_of(key)
    lg, ran = run(clf_of(key, False), x)
    assert LONG <= ran and not (ran & SHORT_ONLY), (key_id(key), sorted(ran))
    empty = ~(x != 0).any(1)
    assert (lg[empty] == 0.0).all()                                           # an all-padding row: logit 0, like the reference
    graded(key, "forward", G.logit_rows(lg, refs_of(key), (K_OF.get(key) or {}).get("logits", G.K)), x, lg)


def embedding_graded(key):
    sd, fe, x, y, w, chrom = batch_of(key)
    got, ran = embed(clf_of(key, False), x)
    assert LONG_EMB <= ran and not (ran & NOT_HERE), (key_id(key), sorted(ran))
    assert_structure(got, x)
    if key not in _EREFS:
        _EREFS[key] = embedding_refs(sd, fe, x)
    rows = grade_rows(got, _EREFS[key], G.K)
    print(f"embedding {key_id(key)}: e/noise " + ", ".join(f"{r.what} {r.ratio:.2f}" for r in rows))
    graded(key, "embedding", rows, x)
    return got


def step_graded(key):
    sd, fe, x, y, w, chrom = batch_of(key)
    case, L = key[0], key[1]
    got, ran = step(clf_of(key, True), x, y, w, np_seed=case[3] + L)
    assert LONG_TRAIN <= ran and not (ran & SHORT_BWD), (key_id(key), sorted(ran))
    graded(key, "step", G.grade(got, refs_of(key), K_OF.get(key)), x, got.logits)
    return got


_every = lambda case, L, kind="every_k": (case, L, kind, "", False)
_EVERY_IDS = [f"{c[0]}-d{c[1]}-{c[2]}-L{L}" for c, L in EVERY_K]


# ---- 1. every width, every k ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,L", EVERY_K, ids=_EVERY_IDS)
def test_every_width_every_k_forward(case, L):
    for kind in ("every_k", "scatter"):
        assert ks_of(batch_of(_every(case, L, kind))[2]) == list(range(L + 1))
        forward_graded(_every(case, L, kind))


@pytest.mark.parametrize("case,L", EVERY_K, ids=_EVERY_IDS)
def test_every_width_every_k_embedding(case, L):
    for kind in ("every_k", "scatter"):                                       # scatter: attn_long_prob_kernel's popcount lookups
        embedding_graded(_every(case, L, kind))


@pytest.mark.parametrize("case,L", EVERY_K, ids=_EVERY_IDS)
def test_every_width_every_k_training_step(case, L):
    step_graded(_every(case, L))


# ---- 2. the multiplicity in closed form -----------------------------------------------------------------------------------------------------------------
_FLAT = {}


def flat_model(case):
    """The case's model with encode1.mul_head_attn.w_ks.weight = 0 (the layer has no bias, Modules.py: nn.Linear(..., bias=False)): every score is 0."""
    if case not in _FLAT:
        sd = dict(batch_of(_every(case, 9))[0])
        name = "encode1.mul_head_attn.w_ks.weight"
        sd[name] = np.zeros_like(sd[name])
        clf, _ = hip_model(synth.LAYOUTS[case[0]], case[1], case[2], case[3], sd=sd)
        assert clf.encode1.mul_head_attn.w_ks.bias is None
        _FLAT[case] = clf.eval()
    return _FLAT[case]


@pytest.mark.parametrize("L", range(9, 33))
@pytest.mark.parametrize("case", [MERGED, FOURPROD], ids=["merged", "fourprod"])
def test_uniform_scores_give_one_over_l_minus_one(case, L):
    """Every score 0: a real query's probability is 1 / (L - 1) at every other slot, real or padding, 0 on the diagonal.  The kernel rounds three
    times (1 / den, the product with n_pad, the product with inv_pad): 4 ulp of float32(1 / (L - 1))."""
    clf = flat_model(case)
    want = np.float32(1.0) / np.float32(L - 1)
    tol = 4.0 * float(np.spacing(want))
    for scatter in (False, True):
        x = batch_of(_every(case, L, "scatter" if scatter else "every_k"))[2]
        got, ran = embed(clf, x)
        assert LONG_EMB <= ran and not (ran & NOT_HERE), sorted(ran)
        attn = got["attn"]                                                    # float64 [8, B, L, L]
        real = x != 0
        off = ~np.eye(L, dtype=bool)
        for b in range(len(x)):
            k = int(real[b].sum())
            blk = attn[:, b]
            assert (blk[:, ~real[b]] == 0.0).all(), (L, k, scatter)           # padding queries; k = 0: the whole block
            assert (blk[:, np.arange(L), np.arange(L)] == 0.0).all(), (L, k, scatter)
            if k:
                dev = np.abs(blk[:, real[b]] - float(want))[:, off[real[b]]]      # [8, k (L - 1)]: the real queries' off-diagonal slots
                assert dev.max() <= tol, (f"L = {L}, k = {k}, scatter {scatter}: {dev.max() / np.spacing(want):.1f} ulp from 1 / (L - 1)",
                                          np.flatnonzero(x[b]).tolist())


# ---- 3. stress, and the embed dims no model was built at ------------------------------------------------------------------------------------------------------
ROW_KEYS = [k for k in KEYS if k[2] == "rows" and not k[4]]
DROP_KEYS = [k for k in KEYS if k[4]]
HOT_KEY = (MERGED, HOT_L, "hot", "hot", False)


@pytest.mark.parametrize("key", ROW_KEYS, ids=key_id)
def test_rows_forward_at_fp32_grade(key):
    x = batch_of(key)[2]
    assert x.shape == (65, key[1]) and ks_of(x)[:5] == [key[1], 2, 1, 0, 9]
    forward_graded(key)


@pytest.mark.parametrize("key", ROW_KEYS, ids=key_id)
def test_rows_embedding_at_fp32_grade(key):
    embedding_graded(key)


@pytest.mark.parametrize("key", ROW_KEYS, ids=key_id)
def test_rows_training_step_at_fp32_grade(key):
    got = step_graded(key)
    assert got.logits[3] == 0.0                                               # the all-padding row


@pytest.mark.parametrize("key", DROP_KEYS, ids=key_id)
def test_saturated_pff_step_with_dropout_at_fp32_grade(key):
    """pff_n1 saturated and dropout on at the model's default p; masks and call seed as test_long_training_step_with_dropout_at_fp32_grade derives
    them.  The control is the same stress dropout-free (test_rows_training_step_at_fp32_grade)."""
    (layout, d, mode, seed), L = key[0], key[1]
    sd, fe, x, y, w, chrom = batch_of(key)
    clf = clf_of(key, True, dropout=True)
    ps = clf._dropout_p()
    assert tuple(round(float(p), 6) for p in ps[1:]) == P_DEFAULT[1:] and clf.training, ps
    rt = clf._runtime()
    call_seed = (int(torch.initial_seed()) * 1000003 + rt.seed_counter + 1) & 0x7FFFFFFFFFFFFFFF
    masks = G.step_masks(call_seed, ps, x.size, d, synth.LAYOUTS[layout] if mode == "adj" else None)
    ref = G.references(sd, fe, x, y, w, chrom=chrom, beta=BETA, masks=masks)
    got, ran = step(clf, x, y, w, np_seed=seed + L)
    assert clf._runtime() is rt and rt.seed_counter >= 1
    assert LONG_TRAIN <= ran and not (ran & SHORT_BWD), sorted(ran)
    RESULTS.setdefault(key_id(key), {})["step, dropout"] = G.assert_grade(f"step, dropout, {key_id(key)}", G.grade(got, ref, K_OF.get(key)))
    assert logit_err(got.logits, refs_of(key[:4] + (False,)).r32a.logits) > 100 * TOL        # (and the masks did something)


def test_hot_node_training_step_at_fp32_grade():
    """About 870 float atomic addends into table row 1; 1 025 hyperedges: the backward's workgroups walk two and three hyperedges each."""
    x = batch_of(HOT_KEY)[2]
    assert x.shape == (HOT_ROWS, HOT_L) and 850 <= int((x[:, 0] == 1).sum()) <= 880 and min(ks_of(x)) >= 2
    step_graded(HOT_KEY)


# ---- 4. the attention backward alone ----------------------------------------------------------------------------------------------------------------------
def _bwd(group, d, shared, L, ks, seed, q_scale=1.0, reference=None):
    r = attention_backward_case(d, shared, L, ks, seed, q_scale=q_scale, pad_row=True, reference=reference)
    worst = BWD_RESULTS.setdefault(group, {})
    for what, v in r.items():
        worst[what] = max(worst.get(what, 0.0), v)


@pytest.mark.parametrize("L", range(2, 33))
@pytest.mark.parametrize("d,shared", [(16, False), (64, True)])
def test_attention_backward_on_the_whole_l_k_grid(d, shared, L):
    _bwd(f"grid d{d} {'shared' if shared else 'per head'}", d, shared, L, list(range(L + 1)), 2000 + d + L)


@pytest.mark.parametrize("L", [9, 17, 32])
@pytest.mark.parametrize("d,shared", [(8, False), (24, False), (40, False), (48, False), (56, False), (192, True), (256, True), (192, False)])
def test_attention_backward_at_every_embed_dim(d, shared, L):
    _bwd(f"dims d{d} {'shared' if shared else 'per head'}", d, shared, L, list(range(L + 1)), 3000 + d + L + (500 if shared else 0))


@pytest.mark.parametrize("L", [17, 32])
@pytest.mark.parametrize("d,shared", [(16, False), (64, True)])
def test_attention_backward_on_sharp_scores(d, shared, L):
    _bwd(f"sharp d{d} {'shared' if shared else 'per head'}", d, shared, L, list(range(L + 1)), 4000 + d + L, q_scale=20.0)    # scores of about +-60


@pytest.mark.parametrize("d,shared", [(16, False), (64, True)])
def test_attention_backward_walks_three_and_four_hyperedges(d, shared):
    """B = 1 537 = 3 x 512 + 1 at L = 9, k in 0 .. 9: every workgroup of the walk takes three hyperedges and one takes four; the padding token's
    dK / dV sums collect in LDS over them.  The torch reference is the batched restatement of torch_attention_grads
    (tests/test_cpu_long_grid.py, equal to it to 1e-13 in fp64): the per-hyperedge loop takes tens of seconds here."""
    ks = [int(k) for k in np.random.default_rng(5000 + d).integers(0, 10, size=1537)]
    assert min(ks) == 0 and max(ks) == 9
    _bwd(f"walk d{d} {'shared' if shared else 'per head'}", d, shared, 9, ks, 5000 + d, reference=torch_attention_grads_by_k)
