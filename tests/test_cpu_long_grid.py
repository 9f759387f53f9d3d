"""The case tables and batch builders of tests/test_hip_long_grid.py (every embed_dim check_shape_fields accepts, every width 9 .. 32 with every k
in one batch, the stresses of tests/fp64_grade.py on the long rows), and, without a GPU, the power of the fp32-grade criterion on every one of
those batches: the fp32 oracle passes G.grade at K = 8 and the three-product witness is rejected by the same bound."""
import numpy as np
import pytest
import torch

from matcha_amd import synth
from tests import fp64_grade as G
from tests.helpers import oracle_state
from tests.test_cpu_long_train import GRADE_CASES, grade_case, predraw_chrom, rows_of

BETA = 0.001
P_DEFAULT = (0.2, 0.3, 0.4)                  # (p_adj, p_fc1, p_pff) of a freshly built Classifier

# (layout, embed_dim, mode, seed): the embed dims check_shape_fields accepts and no other test builds a model at
DIM_CASES = [("tiny", 8, "table", 311), ("tiny", 24, "table", 312), ("tiny", 40, "adj", 313), ("c1", 48, "table", 314), ("c1", 56, "adj", 315),
             ("c1", 192, "table", 316), ("c1", 192, "adj", 319)]     # (seeds 317 and 318 leave the L <= 8 step's witness under 2 x its bound)
DIM_WIDTHS = (17, 32)
DIM_SHARP = (DIM_CASES[2], DIM_CASES[5])
# every k of every width: merged heads (hg38_1mb, 64, table) and the four products (tiny, 16, adj)
MERGED, FOURPROD = GRADE_CASES[0], GRADE_CASES[3]
EVERY_K = [(MERGED, L) for L in range(9, 33)] + [(FOURPROD, L) for L in (9, 12, 16, 17, 20, 24, 28, 31, 32)]
STRESSES = ("small", "sharp", "saturated", "saturated_pff")
STRESS_WIDTHS = (17, 32)
SHARP_ONLY = (GRADE_CASES[1], GRADE_CASES[2])             # (c1, 128, adj), (c1, 256, table)
HOT_ROWS, HOT_L = 1025, 17


def every_k_batch(layout, L, seed, scatter=False):
    """(x, y, w, chrom): rows with k = 0, 1, .., L real ids (B = L + 1), distinct and ascending; with ``scatter`` every third row's ids are spread
    over random slots (the ids keep their order, the pads move inside the row).  Random labels, weights in [0.5, 2); chrom as grade_case."""
    rng = np.random.default_rng(seed + 1000 + L)
    N = int(np.sum(synth.LAYOUTS[layout]))
    ks = list(range(L + 1))
    x = rows_of(rng, N, ks, L)
    if scatter:
        for b in range(0, L + 1, 3):
            row = np.zeros(L, dtype=np.int64)
            row[np.sort(rng.choice(L, size=ks[b], replace=False))] = x[b, :ks[b]]
            x[b] = row
    y = (rng.random(L + 1) < 0.5).astype(np.float32)
    w = (0.5 + 1.5 * rng.random(L + 1)).astype(np.float32)
    return x, y, w, predraw_chrom(len(synth.LAYOUTS[layout]), seed + L)


def hot_batch(layout, seed):
    """(x, y, w, chrom): 1 025 rows at L = 17, k uniform in [2, 17], node 1 in the first slot of 85 % of the rows (about 870 addends into table row 1)."""
    rng = np.random.default_rng(seed + 2000)
    N = int(np.sum(synth.LAYOUTS[layout]))
    x = rows_of(rng, N, [int(k) for k in rng.integers(2, HOT_L + 1, size=HOT_ROWS)], HOT_L)
    y = (rng.random(HOT_ROWS) < 0.5).astype(np.float32)
    w = (0.5 + 1.5 * rng.random(HOT_ROWS)).astype(np.float32)
    return G.hot_node(x, 0.85), y, w, predraw_chrom(len(synth.LAYOUTS[layout]), seed + HOT_L)


def stress(sd, fe, x, w, chrom, name):
    """(sd, x, w) under a stress of tests/fp64_grade.py, the transforms unchanged; ``saturated`` also zeroes every fifth weight, as
    tests/test_hip_fp64_grade.py::_data does."""
    if name == "small":
        return G.small_amplitude(sd), x, w
    if name == "sharp":
        return G.sharp_attention(sd), x, w
    if name == "saturated":
        w = w.copy()
        w[::5] = 0.0
        return G.saturated_logits(sd, fe, x, chrom), x, w
    if name == "saturated_pff":
        return G.saturated_pff(sd, fe, x, chrom), x, w
    if name == "hot":
        return sd, G.hot_node(x, 0.85), w
    assert name == "", name
    return sd, x, w


def torch_attention_grads_by_k(Qn, Kn, Vn, dOn, row_off, L, d, shared, dtype):
    """[dQ, dK, dV] (float64 numpy) of tests/test_hip_long_train.py::torch_attention_grads -- the same mathematics in torch autograd, ``dtype``
    throughout -- with the hyperedges of one k batched into one product each, for batches of more than a thousand hyperedges."""
    Q, K, V = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (Qn, Kn, Vn))
    dO = torch.from_numpy(dOn).to(dtype)
    row_off = np.asarray(row_off, dtype=np.int64)
    T, ks = int(row_off[-1]), np.diff(row_off)
    heads = lambda a, n, k: (a.view(n, k, 1, d) if a.shape[-1] == d else a.view(n, k, 8, d)).permute(0, 2, 1, 3).expand(n, 8, k, d)
    loss = 0.0
    for k in sorted(set(int(v) for v in ks if v > 0)):
        idx = torch.from_numpy(row_off[:-1][ks == k][:, None] + np.arange(k)[None, :])          # [n, k] token rows
        n, n_pad = len(idx), L - k
        q, kk, vv = heads(Q[idx], n, k), heads(K[idx], n, k), heads(V[idx], n, k)
        s = (q @ kk.transpose(-1, -2) / np.sqrt(d)).masked_fill(torch.eye(k, dtype=torch.bool), float("-inf"))
        if n_pad > 0:
            kp, vp = heads(K[T:T + 1], 1, 1), heads(V[T:T + 1], 1, 1)                          # [1, 8, 1, d]
            sp = q @ kp.transpose(-1, -2) / np.sqrt(d) + np.log(n_pad)                          # [n, 8, k, 1]
            s, vv = torch.cat([s, sp], -1), torch.cat([vv, vp.expand(n, 8, 1, d)], 2)
        o = (torch.softmax(s, -1) @ vv).permute(0, 2, 1, 3).reshape(n, k, 8 * d)
        loss = loss + (o * dO[idx]).sum()
    return [g.double().numpy() for g in torch.autograd.grad(loss, [Q, K, V])]


# ---- what the GPU file grades: one key per batch ------------------------------------------------------------------------------------------------------
# key = (case, L, kind, stress, drop): kind "every_k" | "scatter" | "rows" (the 65-row grade_case batch) | "hot"; drop: the step runs with dropout on
def _keys():
    keys = []
    for case, L in EVERY_K:
        keys += [(case, L, "every_k", "", False), (case, L, "scatter", "", False)]
    for case in (MERGED, FOURPROD):
        for L in STRESS_WIDTHS:
            keys += [(case, L, "rows", s, False) for s in STRESSES]
            keys.append((case, L, "rows", "saturated_pff", True))
    for case in SHARP_ONLY:
        keys += [(case, L, "rows", "sharp", False) for L in STRESS_WIDTHS]
    keys.append((MERGED, HOT_L, "hot", "hot", False))
    for case in DIM_CASES:
        keys += [(case, L, "rows", "", False) for L in DIM_WIDTHS]
    for case in DIM_SHARP:
        keys += [(case, L, "rows", "sharp", False) for L in DIM_WIDTHS]
    return keys


KEYS = _keys()

# Batches whose default draw leaves the witness inside the bound on every logit row or on every gradient tensor get another draw here (the power
# test below is a condition on the batch, never on K): key -> offset added to the case's seed for the BATCH only (weights unchanged).
BATCH_SEED_OFFSET = {}
# the default draw's witness logit rows (norm-wise, element-wise) lay at 6.5 / 6.0 (L 9), 7.4 / 2.5 (L 12), 4.4 / 4.7 (L 20) times the noise: L + 1
# rows are few, and at embed_dim 16 the witness's error is a matter of the ids drawn
for _L, _off in ((9, 20000), (12, 20000), (20, 10000)):
    for _kind in ("every_k", "scatter"):
        BATCH_SEED_OFFSET[(FOURPROD, _L, _kind, "", False)] = _off


def key_id(key):
    (layout, d, mode, _), L, kind, s, drop = key
    return "-".join(str(p) for p in (layout, f"d{d}", mode, f"L{L}", kind, s or "plain") + (("drop",) if drop else ()))


_BATCHES = {}


def batch_of(key):
    """(sd, fe, x, y, w, chrom) of a key, stress applied; cached for the module that asks (the arrays are not to be modified)."""
    if key not in _BATCHES:
        (layout, d, mode, seed), L, kind, s, _ = key
        _, fe, sd = oracle_state(synth.LAYOUTS[layout], d, mode, seed)
        bseed = seed + BATCH_SEED_OFFSET.get(key, 0)
        if kind in ("every_k", "scatter"):
            x, y, w, _ = every_k_batch(layout, L, bseed, scatter=(kind == "scatter"))
        elif kind == "hot":
            x, y, w, _ = hot_batch(layout, bseed)
        else:
            x, y, w, _ = grade_case(layout, d, mode, bseed, L)
        chrom = predraw_chrom(len(synth.LAYOUTS[layout]), seed + L)            # what a forward draws after np.random.seed(seed + L)
        if kind != "hot":                                                       # (hot_batch has applied its transform)
            sd, x, w = stress(sd, fe, x, w, chrom, s)
        _BATCHES[key] = (sd, fe, x, y, w, chrom)
    return _BATCHES[key]


def masks_of(key, call_seed, ps=P_DEFAULT):
    """The step's dropout masks for the key's batch (G.step_masks) under the call seed ``call_seed``."""
    (layout, d, mode, _), _, _, _, _ = key
    x = batch_of(key)[2]
    return G.step_masks(call_seed, (ps[0] if mode == "adj" else 0.0, ps[1], ps[2]), x.size, d, synth.LAYOUTS[layout] if mode == "adj" else None)


# ---- the builders ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scatter", [False, True])
@pytest.mark.parametrize("L", [9, 17, 32])
def test_every_k_batch_holds_every_k(L, scatter):
    x, y, w, chrom = every_k_batch("tiny", L, 5, scatter)
    assert x.shape == (L + 1, L) and y.shape == w.shape == (L + 1,) and w.min() >= 0.5 and w.max() < 2.0
    assert [int(k) for k in (x != 0).sum(1)] == list(range(L + 1))
    inside = 0
    for b, row in enumerate(x):
        ids = row[row != 0]
        assert (np.diff(ids) > 0).all() and ids.max(initial=1) <= 64
        moved = bool((np.diff((row != 0).astype(int)) > 0).any())
        assert not moved or (scatter and b % 3 == 0), (b, row)
        inside += moved
    assert (inside >= 2) == scatter
    x2 = every_k_batch("tiny", L, 5, scatter)[0]
    assert np.array_equal(x, x2)


def test_hot_batch_and_stress_transforms():
    x, y, w, _ = hot_batch("hg38_1mb", 191)
    k = (x != 0).sum(1)
    assert x.shape == (HOT_ROWS, HOT_L) and k.min() >= 2 and k.max() == HOT_L
    assert 850 <= int((x == 1).sum()) <= 880 and (x[:, 0] == 1).sum() == (x == 1).sum()
    _, fe, sd = oracle_state(synth.LAYOUTS["tiny"], 16, "adj", 194)
    x, y, w, chrom = grade_case("tiny", 16, "adj", 194, 17)
    for name in STRESSES + ("hot", ""):
        sd2, x2, w2 = stress(sd, fe, x, w, chrom, name)
        changed = sorted(n for n in sd if not np.array_equal(sd[n], sd2[n]))
        assert bool(changed) == (name not in ("hot", "")), (name, changed)
        assert np.array_equal(x, x2) == (name != "hot") and (w2[::5] == 0).all() == (name == "saturated")
    assert w.min() >= 0.5                                                       # (the caller's arrays are left alone)
    assert len(set(KEYS)) == len(KEYS) and set(BATCH_SEED_OFFSET) <= set(KEYS)


@pytest.mark.parametrize("d,shared", [(16, False), (8, True)])
def test_batched_attention_reference_is_the_per_hyperedge_one(d, shared):
    from tests.test_hip_long_train import torch_attention_grads
    L, ks = 9, list(range(10)) + [3, 9, 1, 0, 3]
    row_off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    T, rng = int(row_off[-1]), np.random.default_rng(d)
    Q, dO = (rng.standard_normal((T + 1, 8 * d)).astype(np.float32) for _ in range(2))
    K, V = (rng.standard_normal((T + 1, d if shared else 8 * d)).astype(np.float32) for _ in range(2))
    dO[T] = 0.0
    a = torch_attention_grads(Q, K, V, dO, row_off, L, d, shared, torch.float64)
    b = torch_attention_grads_by_k(Q, K, V, dO, row_off, L, d, shared, torch.float64)
    for name, u, v in zip(("dQ", "dK", "dV"), a, b):
        assert u.shape == v.shape and G.tensor_err(v, u) <= 1e-13, (name, G.tensor_err(v, u))
        assert G.tensor_err(v[T], u[T]) <= 1e-13 or name == "dQ"
    assert not b[0][T].any()


POWER = {}


@pytest.fixture(scope="module", autouse=True)
def _power_table():
    yield
    if POWER:
        print("\nthree-product witness per graded batch: its logit rows' e / noise (norm-wise, element-wise), gradient tensors rejected")
        for name, (lg, bad) in POWER.items():
            print(f"  {name:52s} logits {lg[0]:6.1f} {lg[1]:6.1f}   " + ("forward only" if bad is None else f"{bad[0]} of {bad[1]} rejected"))


# ---- the criterion has power on every graded batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_criterion_has_power_on_every_graded_batch(key):
    """R32a passes G.grade at K = 8; the three-product witness is rejected on at least one logit row and (forward and backward) on at least one
    gradient tensor.  The every-k batches of the width grid run the witness's forward only."""
    sd, fe, x, y, w, chrom = batch_of(key)
    _, L, kind, s, drop = key
    assert x.shape[1] == L
    masks = masks_of(key, 4242 + L) if drop else None
    ref = G.references(sd, fe, x, y, w, chrom=chrom, beta=BETA, masks=masks)
    G.assert_grade(f"R32a {key_id(key)}", G.grade(ref.r32a, ref))
    backward = kind not in ("every_k", "scatter")
    wit = G.oracle_step(sd, fe, x, y, w, chrom=chrom, beta=BETA, ops=G.THREE_PRODUCT, backward=backward, masks=masks)
    lrows = G.logit_rows(wit.logits, ref)
    print(f"witness {key_id(key)}: logits e/noise " + ", ".join(f"{r.ratio:.1f}" for r in lrows))
    POWER[key_id(key)] = ([r.ratio for r in lrows], None)
    assert any(not r.ok for r in lrows), [(r.what, r.ratio) for r in lrows]
    if backward:
        rows = G.grade(wit, ref)
        bad = [r.what for r in rows if not r.ok]
        print(f"witness {key_id(key)}: {len(bad)} of {len(rows)} outputs rejected, worst {max(r.ratio for r in rows):.1f}")
        grads = [n for n in bad if n not in ("logits", "logits (element-wise)", "bce", "recon")]
        POWER[key_id(key)] = ([r.ratio for r in lrows], (len(grads), len(rows) - 4))
        assert grads, bad
