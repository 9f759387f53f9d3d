"""CPU checks of the regression task mode (main.py:60-117): the new C-ABI symbols are declared, exported and bound, an unknown
objective is refused before any device call, and the pairing bijection of matcha_step_record_pairs -- restated here in numpy,
bit for bit -- is a bijection whose pairs depend on (seed, step)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from matcha_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("matcha_forward_objective", "matcha_backward_objective", "matcha_step_record_pairs")

# ---- the pairing bijection of epoch_step.hip (step_record_pairs_kernel), restated in numpy ---------------------------------------------
_U64 = np.uint64
_GOLDEN = 0x9E3779B97F4A7C15


def _mix(v):
    """murmur3's 64-bit finaliser on a uint64 array (wrapping arithmetic)."""
    v = v ^ (v >> _U64(33))
    v = v * _U64(0xff51afd7ed558ccd)
    v = v ^ (v >> _U64(33))
    v = v * _U64(0xc4ceb9fe1a85ec53)
    return v ^ (v >> _U64(33))


def pair_key(seed: int, step: int) -> np.ndarray:
    s = np.array([(int(step) + _GOLDEN) & 0xFFFFFFFFFFFFFFFF], dtype=_U64)
    return _mix(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=_U64) ^ _mix(s))


def pair_permutation(B: int, seed: int, step: int) -> np.ndarray:
    """pi as int64 [B]: a 6-round balanced Feistel network on [0, 2^m) (m even, 2^m >= B) keyed by (seed, step), walked in cycles
    until it lands in [0, B)."""
    m = 2
    while (1 << m) < B:
        m += 2
    hb = _U64(m // 2)
    mask = _U64((1 << (m // 2)) - 1)
    key = pair_key(seed, step)
    v = np.arange(B, dtype=_U64)
    todo = np.arange(B)
    while todo.size:
        lo, hi = v[todo] >> hb, v[todo] & mask
        for r in range(6):
            f = _mix(key ^ (_U64(r) << _U64(32)) ^ hi) & mask
            lo, hi = hi, lo ^ f
        v[todo] = (lo << hb) | hi
        todo = todo[v[todo] >= _U64(B)]
    return v.astype(np.int64)


def pair_records(logits, y, x, seed: int, step: int):
    """What matcha_step_record_pairs writes for one step: (preds [B/2] float64, labels [B/2] int32, sizes [B/2] int64)."""
    B = len(y)
    pi = pair_permutation(B, seed, step)
    r0, r1 = pi[0:2 * (B // 2):2], pi[1:2 * (B // 2):2]
    sp = np.where(logits > 20, logits.astype(np.float64), np.log1p(np.exp(logits.astype(np.float64))))
    preds = 1.0 / (1.0 + np.exp(-(sp[r0] - sp[r1])))
    labels = np.where(y[r0] == y[r1], -1, np.where(y[r1] < y[r0], 1, 0)).astype(np.int32)
    sizes = (x[r0] != 0).sum(1).astype(np.int64)
    return preds, labels, sizes


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "matcha_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert re.search(r"#define MATCHA_OBJECTIVE_BCE 0\b", src) and re.search(r"#define MATCHA_OBJECTIVE_SOFTPLUS_MSE 1\b", src)
    assert (_lib.OBJECTIVE_BCE, _lib.OBJECTIVE_SOFTPLUS_MSE) == (0, 1)
    assert lib.matcha_abi_version() == _lib.ABI_VERSION == 7


@pytest.mark.parametrize("fn", ["matcha_forward_objective", "matcha_backward_objective"])
@pytest.mark.parametrize("objective", [7, -1, 2])
def test_unknown_objective_is_refused_before_any_device_call(fn, objective):
    """Null pointers everywhere: the objective check must come first (no device call, no dereference)."""
    lib = _lib.load()
    n_args = len(_lib.SIGNATURES[fn][1]) - 1
    args = [None] * n_args
    args[5], args[6] = 4, 2                    # B, L
    args[-2] = 0                               # ws_bytes
    rc = getattr(lib, fn)(objective, *args)
    assert rc == -22                           # MATCHA_EINVAL
    assert "objective" in lib.matcha_last_error().decode()


def test_step_record_pairs_checks_its_arguments():
    lib = _lib.load()
    assert lib.matcha_step_record_pairs(None, None, None, None, 4, 2, None, 1, None, None, None, None, None, None) == -22
    assert "matcha_step_record_pairs" in lib.matcha_last_error().decode()


def test_trainer_refuses_an_unknown_objective():
    from matcha_amd.engine import Trainer
    with pytest.raises(ValueError, match="objective"):
        Trainer.__init__(object.__new__(Trainer), None, objective="rank")


@pytest.mark.parametrize("B", [2, 3, 192, 384, 65536])
def test_pair_permutation_is_a_bijection(B):
    for seed, step in ((0, 0), (12345, 7), (1 << 61, 199)):
        pi = pair_permutation(B, seed, step)
        assert pi.dtype == np.int64 and len(pi) == B
        assert np.array_equal(np.sort(pi), np.arange(B))


def test_pairs_depend_on_seed_and_step():
    B = 384
    base = pair_permutation(B, 5, 0)
    assert not np.array_equal(base, pair_permutation(B, 5, 1))
    assert not np.array_equal(base, pair_permutation(B, 6, 0))
    assert np.array_equal(base, pair_permutation(B, 5, 0))
    # a fresh draw per step: over 50 steps the first pair's rows are all over the batch
    firsts = {int(pair_permutation(B, 5, s)[0]) for s in range(50)}
    assert len(firsts) > 35


def test_pairing_is_close_to_uniform():
    """The chance that two given rows are paired is 1 / (B - 1) under a uniform matching; 4 000 draws of B = 8 land within 5 sigma of it
    for every one of the 28 row pairs."""
    B, n = 8, 4000
    cnt = np.zeros((B, B))
    for s in range(n):
        pi = pair_permutation(B, 99, s)
        for j in range(B // 2):
            a, b = pi[2 * j], pi[2 * j + 1]
            cnt[a, b] += 1
            cnt[b, a] += 1
    p = 1.0 / (B - 1)
    sig = np.sqrt(n * p * (1 - p))
    off = cnt[~np.eye(B, dtype=bool)]
    assert np.all(np.abs(off - n * p) < 5 * sig), off


def test_pair_records_follow_the_reference_pair_semantics():
    """main.py:94-117 on one pair list: argmin of the two targets, masked when they are equal, sigmoid of the softplus difference."""
    logits = np.array([0.5, -1.0, 25.0, 3.0], dtype=np.float32)
    y = np.array([2.0, 0.0, 0.0, 0.0], dtype=np.float32)
    x = np.array([[1, 2, 0], [3, 4, 5], [6, 7, 0], [8, 9, 10]])
    preds, labels, sizes = pair_records(logits, y, x, 3, 0)
    pi = pair_permutation(4, 3, 0)
    for j in range(2):
        a, b = pi[2 * j], pi[2 * j + 1]
        yy = torch.tensor([[y[a], y[b]]])
        pr = torch.nn.functional.softplus(torch.tensor([[logits[a], logits[b]]], dtype=torch.float64))
        mask = bool(yy[0, 0] != yy[0, 1])
        assert labels[j] == (int(torch.argmin(yy, dim=-1)) if mask else -1)
        assert abs(preds[j] - float(torch.sigmoid(pr[0, 0] - pr[0, 1]))) < 1e-12
        assert sizes[j] == (x[a] != 0).sum()


def test_softplus_mse_gradient_formula():
    """The logit gradient the kernels use, alpha * 2 (softplus(z) - y) softplus'(z) / B with torch's threshold, against autograd."""
    z = torch.tensor([-30.0, -3.0, 0.0, 2.5, 19.9, 20.0, 20.5, 40.0], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([0.0, 1.5, 0.0, 3.0, 19.0, 0.0, 22.0, 41.0], dtype=torch.float64)
    alpha = 0.7
    (alpha * torch.nn.functional.mse_loss(torch.nn.functional.softplus(z), y)).backward()
    zz = z.detach()
    sp = torch.where(zz > 20, zz, torch.log1p(torch.exp(zz)))
    dsp = torch.where(zz > 20, torch.ones_like(zz), torch.sigmoid(zz))
    assert torch.allclose(z.grad, alpha * 2 * (sp - y) * dsp / len(z), rtol=1e-12, atol=1e-15)


# ---- the gr_* fixtures of the REAL reference (tests/golden/make_golden_regress.py): forward_op_batch_regress with y given -----------------
# name -> (layout, embed_dim, front end, weight seed)
GR = {"tiny_table": ("tiny", 64, "table", 101), "tiny_adj": ("tiny", 64, "adj", 102), "hg38_table_d64": ("hg38_1mb", 64, "table", 103),
      "hg38_adj_d64": ("hg38_1mb", 64, "adj", 104), "c1_table_d128": ("c1", 128, "table", 105)}
GAUGE = "encode1.mul_head_attn.layer_norm2.bias"    # see tests/test_oracle_golden.py


def gr_n_steps(g):
    return len(g["alpha"])


def gr_ref(g, prefix, name):
    """(stride, stored elements) of one tensor of a gr_* fixture: in full (stride 1) or every stride-th element of the flattened tensor."""
    if f"{prefix}/{name}" in g.files:
        return 1, g[f"{prefix}/{name}"].reshape(-1)
    for key in g.files:
        head, _, tail = key.partition("/")
        if tail == name and head.startswith(prefix + "s") and head[len(prefix) + 1:].isdigit():
            return int(head[len(prefix) + 1:]), g[key]
    return None, None


def gr_pairs(logits, y):
    """main.py:92-117 with y given (no shuffle): rows (2j, 2j+1) paired, pairs with equal targets dropped; (pred, label)."""
    yy = y.reshape(-1, 2)
    sp = torch.nn.functional.softplus(logits.reshape(-1, 2))
    keep = yy[:, 0] != yy[:, 1]
    return torch.sigmoid(sp[keep, 0] - sp[keep, 1]), torch.argmin(yy, dim=-1)[keep].float()


@pytest.mark.parametrize("name", sorted(GR))
def test_oracle_restatement_reproduces_the_regress_fixtures(name):
    """oracle.hypersagnn + softplus / mse_loss + the pair view, with the oracle's AdamW, against the reference's own regress steps: logits,
    softplus, MSE, recon, the pair outputs, the grad-None set and every stored gradient element of step 0 (2e-5), the parameters after
    the first and the last step."""
    from matcha_amd import synth
    from oracle import hypersagnn as O
    from tests.helpers import gold, oracle_state
    layout, d, mode, seed = GR[name]
    g = gold(f"gr_{name}.npz")
    P, fe, _ = oracle_state(synth.LAYOUTS[layout], d, mode, seed, requires_grad=True)
    opt = O.AdamWRef()
    names = [n for n, t in P.items() if t.requires_grad]
    n_steps = gr_n_steps(g)
    cats = set()
    for step in range(n_steps):
        x, y = torch.from_numpy(g[f"x{step}"].astype(np.int64)), torch.from_numpy(g[f"y{step}"])
        alpha, beta = float(g["alpha"][step]), float(g["beta"][step])
        logits, recon = O.classifier_forward(P, fe, x, random_chrom=int(g["chroms"][step]))
        mse = torch.nn.functional.mse_loss(torch.nn.functional.softplus(logits), y)
        grads = dict(zip(names, torch.autograd.grad(mse * alpha + recon * beta, [P[n] for n in names], allow_unused=True)))
        lg = logits.detach()
        scale = max(float(np.abs(g[f"logits{step}"]).max()), 1e-3)
        assert float(np.abs(lg.numpy() - g[f"logits{step}"]).max()) <= 2e-5 * scale, step
        assert np.abs(torch.nn.functional.softplus(lg).numpy() - g[f"sp{step}"]).max() <= 2e-5 * max(float(np.abs(g[f"sp{step}"]).max()), 1.0)
        assert abs(float(mse.detach()) - float(g[f"mse{step}"])) <= 2e-5 * max(1.0, float(g[f"mse{step}"])), step
        assert abs(float(recon.detach()[0]) - float(g[f"recon{step}"][0])) <= 2e-5 * max(1.0, abs(float(g[f"recon{step}"][0]))), step
        pp, pl = gr_pairs(lg, y)
        assert np.array_equal(pl.numpy(), g[f"pair_y{step}"]), step
        assert np.abs(pp.numpy() - g[f"pair_pred{step}"]).max() <= 2e-5, step
        assert np.all(g[f"pair_s{step}"] == 1.0)                     # main.py:74: s = ones when y is given
        yy = g[f"y{step}"].reshape(-1, 2)
        cats |= {(bool(a > 0), bool(b > 0), bool(a == b)) for a, b in yy}
        if step == 0:
            assert {n for n, v in grads.items() if v is None} == set(g["grad_none"].tolist()) - {"attribute_dict_embedding.weight"}
            checked = 0
            for n, v in grads.items():
                if v is None or n == GAUGE:
                    continue
                stride, ref = gr_ref(g, "grad0", n)
                got = v.numpy().reshape(-1)[::stride]
                assert np.abs(got - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1e-3), n
                checked += 1
            assert checked >= 20
        opt.step(P, grads)
        if step in (0, n_steps - 1):
            checked = 0
            for n in names:
                stride, ref = gr_ref(g, f"param{step}", n)
                if stride is None:
                    continue
                got = P[n].detach().numpy().reshape(-1)[::stride]
                if n == GAUGE:
                    assert np.abs(got - ref).max() <= 1.1e-3 * (step + 1) + 1e-6
                    continue
                assert np.abs(got - ref).max() <= 5e-5 * max(np.abs(ref).max(), 1e-3), (step, n)
                checked += 1
            assert checked >= 20
    # every pair category occurs: pos-neg, neg-pos, neg-neg, pos-pos equal, pos-pos distinct
    assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True), (True, True, False)} <= cats


def test_session_pairwise_and_cli_refuse_an_unknown_mode():
    from matcha_amd import predict as PR
    from matcha_amd import train as T
    with pytest.raises(ValueError, match="task_mode"):
        T.Session(None, None, None, 2, 3, 0, task_mode="rank")
    with pytest.raises(ValueError, match="task_mode"):
        PR.pairwise_probabilities(None, None, 0, 0, task_mode="rank")
    with pytest.raises(SystemExit):
        T.main(["--task-mode", "rank"])
    with pytest.raises(SystemExit):
        PR.main(["pairwise", "--chrom", "0", "--task-mode", "rank"])
