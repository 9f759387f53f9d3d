"""Classifier.get_embedding on rows of 9 to 32 columns on the device (matcha_get_embedding_long; attn_long_prob_kernel): parity with the real
reference's outputs (tests/golden/g14_long_embedding.npz), fp32 grade against the fp64 oracle (tests/fp64_grade.py::row as it is, K = 8) on
attn, dynamic and static, the exact structure of the attention tensor, the same O bits with and without the probabilities, the long entry
point beside the L <= 8 path, shape edges, the row's width, refusals, the untouched paths, get_node_embeddings on wide input and the
`predict attention` consumer.  GPU only (-m gpu)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from matcha_amd import _lib, predict as PR, synth
from tests import fp64_grade as G
from tests.helpers import GOLD, gold
from tests.test_cpu_long_embedding import (OUTPUTS, WIDTHS, embedding_batch, embedding_refs, fixture_case, grade_rows, oracle_embedding,
                                           witness)
from tests.test_hip_long_rows import GRADE_CASES, LONG_PLAN, SHORT_ONLY, model, rows_of
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

PROB = "attn_long_prob_kernel"
LONG_EMB = LONG_PLAN | {PROB, "expand_embedding_kernel"}
NOT_HERE = {"attn_long_kernel", "attn_fwd_kernel", "attn_fwd_wide_kernel", "fused_fwd32_kernel", "fused_fwd32h_kernel", "enc128_fwd_kernel"}
EDGE = ("hg38_1mb", 64, "table", 181)


def as_outputs(dyn, sta, attn, B, L):
    """float64 numpy {attn [8, B, L, L], dynamic, static [B, L, d]} of the three device tensors."""
    assert attn.shape == (8 * B, L, L) and dyn.shape == sta.shape and dyn.shape[:2] == (B, L)
    return {"attn": attn.cpu().numpy().astype(np.float64).reshape(8, B, L, L), "dynamic": dyn.cpu().numpy().astype(np.float64),
            "static": sta.cpu().numpy().astype(np.float64)}


def embed(clf, x):
    """({attn, dynamic, static}, kernels) of clf.get_embedding(x) under no_grad."""
    with torch.no_grad(), _lib.launch_log() as log:
        dyn, sta, attn = clf.get_embedding(torch.from_numpy(x))
        torch.cuda.synchronize()
    return as_outputs(dyn, sta, attn, *x.shape), {k for k, n in log.counts.items() if n > 0}


def c_embed(clf, x, with_attn=True, training=0):
    """matcha_get_embedding_long called directly on NaN-filled outputs: (rc, device tensors (dyn, sta, attn), kernels)."""
    rt = clf._runtime()
    with torch.no_grad():
        opts, _ = clf._opts(rt, False)
    opts.training, opts.forward_only = training, 1
    opts.status = rt.status.data_ptr()
    xt = torch.from_numpy(x).cuda().contiguous()
    B, L = xt.shape
    ws = rt.workspace(B, L, long_rows=True)
    dyn = torch.full((B, L, rt.d), float("nan"), dtype=torch.float32, device="cuda")
    sta = torch.full_like(dyn, float("nan"))
    attn = torch.full((8 * B, L, L), float("nan"), dtype=torch.float32, device="cuda")
    with _lib.launch_log() as log:
        rc = rt.lib.matcha_get_embedding_long(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xt), B, L, _lib.ptr(dyn),
                                              _lib.ptr(sta), _lib.ptr(attn) if with_attn else None, None, _lib.ptr(ws), ws.numel(), rt.stream())
        torch.cuda.synchronize()
    return rc, (dyn, sta, attn), {k for k, n in log.counts.items() if n > 0}


def assert_case1_bounds(label, got, ref, x):
    """The bounds of test_get_embedding_matches_oracle_intermediates: dynamic within 1e-4 of max|dynamic|, static within 1e-5, attn within 1e-5
    (absolute) with the rows of padding queries masked.  ``ref``: {attn [8, B, L, L], dynamic, static}."""
    qmask = (x != 0).astype(np.float64)[None, :, :, None]
    e_dyn = float(np.abs(got["dynamic"] - ref["dynamic"]).max()) / max(float(np.abs(ref["dynamic"]).max()), 1e-30)
    e_sta = float(np.abs(got["static"] - ref["static"]).max())
    e_attn = float(np.abs(got["attn"] - ref["attn"] * qmask).max())
    print(f"{label}: dynamic {e_dyn:.2e} of max, static {e_sta:.2e}, attn {e_attn:.2e}")
    assert e_dyn <= 1e-4 and e_sta <= 1e-5 and e_attn <= 1e-5, (label, e_dyn, e_sta, e_attn)


def assert_structure(got, x):
    """What holds exactly, whatever the weights."""
    attn, dyn = got["attn"], got["dynamic"]
    B, L = x.shape
    real = x != 0
    assert np.isfinite(attn).all() and np.isfinite(dyn).all() and np.isfinite(got["static"]).all()
    assert (attn[:, :, np.arange(L), np.arange(L)] == 0.0).all()                       # the diagonal
    assert (attn[:, ~real] == 0.0).all()                                               # rows of padding queries
    assert (dyn[~real] == 0.0).all()                                                   # padding slots of dynamic
    empty = ~real.any(1)
    assert (attn[:, empty] == 0.0).all() and (dyn[empty] == 0.0).all()                 # k = 0: the whole block
    sums = attn.sum(-1)                                                                # float64
    assert np.abs(sums - 1.0)[:, real].max() <= 2e-6, float(np.abs(sums - 1.0)[:, real].max())
    first_pad = np.where(real, L, np.arange(L)[None, :]).min(1)                        # a row's first padding slot (L: none)
    for b in np.flatnonzero((~real).sum(1) > 1):
        cols = attn[:, b][:, real[b]][:, :, ~real[b]]
        assert (cols == attn[:, b][:, real[b]][:, :, first_pad[b]:first_pad[b] + 1]).all(), b     # bitwise equal: float64 of float32 is exact


# ---- 1. reference parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["table", "adj"])
def test_reference_parity_of_the_long_embedding(mode):
    import Modules  # noqa: F401  (the pickle's GLOBALs are Modules.*)
    g = gold("g14_long_embedding.npz")
    clf = torch.load(os.path.join(GOLD, f"ref_model2load_tiny_{mode}"), map_location="cuda", weights_only=False).eval()
    for L in WIDTHS:
        x, dyn, sta, attn = fixture_case(g, mode, L)
        got, ran = embed(clf, x)
        assert_case1_bounds(f"{mode} L {L}", got, {"attn": attn.astype(np.float64), "dynamic": dyn, "static": sta}, x)
        assert_structure(got, x)
        assert LONG_EMB <= ran and not (ran & NOT_HERE), sorted(ran)
    # the quadruple: the reconstruction loss of model(x, return_recon=True) under the same draw, and exactly one draw per call
    xt = torch.from_numpy(fixture_case(g, mode, 17)[0])
    with torch.no_grad():
        np.random.seed(3)
        out = clf.get_embedding(xt, None, None, return_recon=True)
        after = np.random.random()
        np.random.seed(3)
        _, recon = clf(xt, return_recon=True)
    assert len(out) == 4 and out[3].shape == (1,) and torch.allclose(out[3], recon, rtol=1e-5, atol=1e-7)
    np.random.seed(3)
    if mode == "adj":
        np.random.choice(np.arange(len(synth.LAYOUTS["tiny"])), 1)
    assert after == np.random.random()


# ---- 2. fp32 grade, 3. structure ------------------------------------------------------------------------------------------------------------------
_GRADED = {}


def graded_case(layout, d, mode, seed, L):
    key = (layout, d, mode, seed, L)
    if key not in _GRADED:
        clf, sd, fe = model(layout, d, mode, seed)
        x = embedding_batch(np.random.default_rng(seed + L), int(np.sum(synth.LAYOUTS[layout])), L)
        got, ran = embed(clf, x)
        assert LONG_EMB <= ran and not (ran & NOT_HERE), sorted(ran)
        _GRADED[key] = (x, got, sd, fe)
    return _GRADED[key]


@pytest.mark.parametrize("L", [9, 32])
@pytest.mark.parametrize("layout,d,mode,seed", GRADE_CASES)
def test_long_embedding_at_fp32_grade(layout, d, mode, seed, L):
    x, got, sd, fe = graded_case(layout, d, mode, seed, L)
    assert x.shape == (65, L) and [int(k) for k in (x[:5] != 0).sum(1)] == [L, 2, 1, 0, 9]
    refs = embedding_refs(sd, fe, x)
    rows = grade_rows(got, refs, G.K)
    print(f"long embedding {layout} d{d} {mode} L{L}: e/noise " + ", ".join(f"{r.what} {r.ratio:.2f}" for r in rows))
    G.assert_grade(f"long embedding {layout} d{d} {mode} L{L}", rows)
    wit = grade_rows(witness(sd, fe, x), refs, G.K)
    print("witness e/noise", [round(r.ratio, 1) for r in wit])
    assert not any(r.ok for r in wit), [(r.what, r.ratio) for r in wit]


@pytest.mark.parametrize("L", [9, 32])
@pytest.mark.parametrize("layout,d,mode,seed", GRADE_CASES)
def test_structure_is_exact(layout, d, mode, seed, L):
    x, got, _, _ = graded_case(layout, d, mode, seed, L)
    assert (x[3] == 0).all() and (np.diff((x != 0).astype(int), axis=1) > 0).any()     # a k = 0 row, pads inside rows
    assert_structure(got, x)


# ---- 4. the same O bits ---------------------------------------------------------------------------------------------------------------------------
def mixed_rows(rng, N, L, B=257):
    ks = [L, 2, 1, 0] + [int(k) for k in rng.integers(1, L + 1, size=B - 4)]
    return rows_of(rng, N, ks, L)


@pytest.mark.parametrize("layout,d,mode,seed", [EDGE, ("tiny", 16, "adj", 184)])
def test_same_outputs_with_and_without_the_probabilities(layout, d, mode, seed):
    clf, sd, fe = model(layout, d, mode, seed)
    x = mixed_rows(np.random.default_rng(seed + 417), int(np.sum(synth.LAYOUTS[layout])), 17)
    rc1, (dyn1, sta1, attn1), ran1 = c_embed(clf, x, with_attn=True)
    rc0, (dyn0, sta0, attn0), ran0 = c_embed(clf, x, with_attn=False)
    assert rc1 == 0 and rc0 == 0
    assert torch.equal(dyn1, dyn0) and torch.equal(sta1, sta0) and not torch.isnan(dyn1).any() and not torch.isnan(sta1).any()
    assert PROB in ran1 and "attn_long_kernel" not in ran1
    assert "attn_long_kernel" in ran0 and PROB not in ran0 and torch.isnan(attn0).all()
    assert not torch.isnan(attn1).any()                                                # every element was written over the NaN fill


# ---- 5. against the short path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,d,mode,seed", [("hg38_1mb", 64, "table", 181), ("c1", 128, "adj", 182)])
@pytest.mark.parametrize("L", [8, 5])
def test_long_entry_point_against_the_short_path(layout, d, mode, seed, L):
    clf, sd, fe = model(layout, d, mode, seed)
    x = mixed_rows(np.random.default_rng(seed + 40 + L), int(np.sum(synth.LAYOUTS[layout])), L)
    refs = embedding_refs(sd, fe, x)
    rc, (dyn, sta, attn), ran_l = c_embed(clf, x)
    assert rc == 0 and LONG_EMB <= ran_l and not (ran_l & NOT_HERE), sorted(ran_l)
    got_l = as_outputs(dyn, sta, attn, *x.shape)
    got_s, ran_s = embed(clf, x)
    assert not (ran_s & (LONG_PLAN | {PROB, "attn_long_kernel"})), sorted(ran_s)
    assert_structure(got_l, x)
    G.assert_grade(f"long entry {layout} d{d} L{L}", grade_rows(got_l, refs, G.K))
    G.assert_grade(f"short path {layout} d{d} L{L}", grade_rows(got_s, refs, G.K))


# ---- 6. shapes where the kernel can go wrong ----------------------------------------------------------------------------------------------------------
def _against_oracle(label, x):
    clf, sd, fe = model(*EDGE)
    got, ran = embed(clf, x)
    assert LONG_EMB <= ran and not (ran & NOT_HERE), sorted(ran)
    assert_case1_bounds(label, got, oracle_embedding(sd, fe, x), x)
    assert_structure(got, x)
    return got


def _N():
    return int(np.sum(synth.LAYOUTS[EDGE[0]]))


@pytest.mark.parametrize("B", [1, 3, 64, 65, 257])
def test_batch_sizes_at_width_17(B):
    rng = np.random.default_rng(1400 + B)
    ks = ([17] + [int(k) for k in rng.integers(1, 18, size=B - 1)])[:B]
    _against_oracle(f"B {B} L 17", rows_of(rng, _N(), ks, 17))


def test_full_rows_1031_by_32():
    rng = np.random.default_rng(1432)
    x = np.sort(np.argsort(rng.random((1031, _N())), axis=1)[:, :32] + 1, axis=1).astype(np.int64)
    _against_oracle("B 1031 L 32 k 32", x)


def test_one_long_row_among_short_ones():
    rng = np.random.default_rng(1425)
    ks = [3] * 300
    ks[170] = 25
    _against_oracle("B 300 L 25, one long row", rows_of(rng, _N(), ks, 25))


def test_pads_inside_rows_repeated_ids_empty_runs_and_the_k_edges():
    rng = np.random.default_rng(1417)
    L, B, N = 17, 300, _N()
    ks = [1, L - 1, L] + [int(k) for k in rng.integers(1, L + 1, size=B - 3)]            # k = 1: the padding slots only; one padding slot; none
    x = rows_of(rng, N, ks, L)
    for b in range(3, B, 3):                                  # pads anywhere in the row: the real ids keep their order, the slots move
        slots = np.sort(rng.choice(L, size=ks[b], replace=False))
        row = np.zeros(L, dtype=np.int64)
        row[slots] = x[b, :ks[b]]
        x[b] = row
    x[4, :4] = [7, 9, 9, 30]                                  # a repeated id in a row
    x[5, :L] = np.sort(rng.choice(N, size=L, replace=False) + 1)
    x[5, 5] = x[5, 11]                                        # ... and in a full row, out of order
    x[7] = 0
    x[7, L - 1] = 11                                          # k = 1 in the LAST slot
    x[8] = x[1]
    x[8, 0], x[8, L - 1] = 0, x[1, 0]                         # k = L - 1 with its padding slot in front
    x[100:170] = 0                                            # a run of 70 all-padding rows in the middle of the batch
    got = _against_oracle("pads inside rows, repeated ids, empty run, k = 1 / L - 1 / L", x)
    assert (got["attn"][:, 100:170] == 0.0).all()
    # k = 1: the query's whole weight lies on the padding slots, equally
    assert (got["attn"][:, 0, 0, 1:] == np.float32(1.0) / np.float32(L - 1)).all() and (got["attn"][:, 0, 0, 0] == 0.0).all()


# ---- 7. the width is honoured -----------------------------------------------------------------------------------------------------------------------
def test_width_is_honoured():
    clf, sd, fe = model(*EDGE)
    rng = np.random.default_rng(1505)
    base = rows_of(rng, _N(), [9] + [int(k) for k in rng.integers(2, 10, size=63)], 9)
    oracle = {}
    for L in (9, 16, 32):
        x = np.pad(base, ((0, 0), (0, L - 9)))
        got, _ = embed(clf, x)
        oracle[L] = oracle_embedding(sd, fe, x)
        assert_case1_bounds(f"width {L}", got, oracle[L], x)
    for a, b in ((9, 16), (16, 32), (9, 32)):                 # asserted on the oracle's numbers: a width-blind output cannot pass all three widths
        gap = float(np.abs(oracle[a]["attn"][:, :, :9, :9] - oracle[b]["attn"][:, :, :9, :9]).max())
        print(f"width {a} vs {b}: attn differs by {gap:.3f}")
        assert gap > 100 * 1e-5, (a, b, gap)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    clf, sd, fe = model(*EDGE)
    N = _N()
    rng = np.random.default_rng(1606)
    x = rows_of(rng, N, [9, 4, 12, 2], 12)
    with _lib.launch_log() as log:
        clf.train()
        try:
            with torch.no_grad(), pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
                clf.get_embedding(torch.from_numpy(x))
        finally:
            clf.eval()
        with torch.no_grad(), pytest.raises(ValueError, match="32"):
            clf.get_embedding(torch.zeros(2, 33, dtype=torch.long))
    assert not log.counts, log.counts
    rc, (dyn, sta, attn), ran = c_embed(clf, x, training=1)
    assert rc == -22 and not ran and torch.isnan(dyn).all() and torch.isnan(attn).all()
    assert "inference-only" in _lib.load().matcha_last_error().decode()
    bad = x.copy()
    bad[2, 7] = N + 1
    with torch.no_grad():
        with pytest.raises(IndexError):
            clf.get_embedding(torch.from_numpy(bad))
        clf.get_embedding(torch.from_numpy(x))                # the status word was cleared
        with pytest.raises(IndexError):
            with clf.deferred_id_check():
                clf.get_embedding(torch.from_numpy(bad))      # no read-back here ...
                out = clf.get_embedding(torch.from_numpy(x))  # ... nor here: raised at the end of the block
        assert out[2].shape == (32, 12, 12)


# ---- 9. nothing else moved ------------------------------------------------------------------------------------------------------------------------
def test_other_paths_run_no_new_kernel():
    clf, sd, fe = model(*EDGE)
    rng = np.random.default_rng(1707)
    _, ran = embed(clf, rows_of(rng, _N(), [8, 2, 5, 3], 8))
    assert not (ran & (LONG_PLAN | {PROB, "attn_long_kernel"})) and ran & {"attn_fwd_kernel", "attn_fwd_wide_kernel"}, sorted(ran)
    x12 = torch.from_numpy(rows_of(rng, _N(), [12, 2, 9, 3], 12))
    with torch.no_grad(), _lib.launch_log() as log:
        clf(x12)
        torch.cuda.synchronize()
    assert "attn_long_kernel" in log.counts and PROB not in log.counts and "expand_embedding_kernel" not in log.counts, log.counts
    trn, _ = hip_model(synth.LAYOUTS["tiny"], 16, "table", 1709)
    trn.long_row_training = True
    trn.train()
    xs = torch.from_numpy(rows_of(rng, int(np.sum(synth.LAYOUTS["tiny"])), [12, 2, 9, 3], 12))
    with _lib.launch_log() as log:
        trn(xs).sum().backward()
        torch.cuda.synchronize()
    assert {"attn_long_kernel", "attn_long_bwd_kernel"} <= set(log.counts) and PROB not in log.counts and "expand_embedding_kernel" not in log.counts


# ---- 10. get_node_embeddings on wide input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,d,mode,seed", [("tiny", 16, "adj", 184), ("c1", 128, "adj", 182), ("hg38_1mb", 64, "table", 181)])
def test_node_embeddings_take_twelve_columns(layout, d, mode, seed):
    clf, sd, fe = model(layout, d, mode, seed)
    x = torch.from_numpy(mixed_rows(np.random.default_rng(seed + 12), int(np.sum(synth.LAYOUTS[layout])), 12, B=37))
    with torch.no_grad():
        wide = clf.get_node_embeddings(x)
        flat = clf.get_node_embeddings(x.reshape(-1, 1))
    assert wide.shape == (37, 12, d) and torch.equal(wide.reshape(-1, d), flat.reshape(-1, d)) and torch.isfinite(wide).all()


# ---- 11. the consumer -----------------------------------------------------------------------------------------------------------------------------
def test_predict_attention_cli(tmp_path):
    import Modules  # noqa: F401
    g = gold("g6_inference_tiny.npz")
    bin2node = {str(k): int(v) for k, v in zip(g["bin_keys"], g["bin_vals"])}
    node2bin = {v: k for k, v in bin2node.items()}
    names, res = [str(n) for n in g["names"]], int(g["res"])
    N = int(np.sum(synth.LAYOUTS["tiny"]))
    rng = np.random.default_rng(1808)
    sizes = [25, 2, 9] + [int(k) for k in rng.integers(2, 26, size=20)]
    lines = [np.sort(rng.choice(N, size=k, replace=False) + 1) for k in sizes]

    def write(path, rows):
        with open(path, "w") as f:
            for r in rows:
                f.write("\t".join(node2bin[int(v)] for v in rng.permutation(r)) + "\n")

    temp = os.path.join(tmp_path, "Temp")
    os.makedirs(temp)
    shutil.copy(os.path.join(GOLD, "ref_model2load_tiny_table"), os.path.join(temp, "model2load"))
    np.save(os.path.join(temp, "bin2node.npy"), bin2node, allow_pickle=True)
    cpath = os.path.join(tmp_path, "config.JSON")
    with open(cpath, "w") as f:
        json.dump({"temp_dir": temp, "resolution": res, "chrom_list": names, "min_distance": 2}, f)
    inp, out = os.path.join(tmp_path, "in.txt"), os.path.join(tmp_path, "attn.npz")
    write(inp, lines)
    PR.main(["attention", "-i", inp, "-o", out, "--per-head", "--config", cpath])
    z = np.load(out)
    assert sorted(z.files) == ["attn_heads", "attn_mean", "offsets", "sizes"]
    assert z["sizes"].tolist() == sizes and z["offsets"].tolist() == np.concatenate([[0], np.cumsum(np.square(sizes))]).tolist()
    assert z["attn_mean"].shape == (z["offsets"][-1],) and z["attn_heads"].shape == (8 * z["offsets"][-1],)
    # one chunk, width 25: each block is the head mean of get_embedding's real slots on that chunk
    clf = torch.load(os.path.join(temp, "model2load"), map_location="cuda", weights_only=False).eval()
    x = np.zeros((len(lines), 25), dtype=np.int64)
    for i, r in enumerate(lines):
        x[i, :len(r)] = r
    with torch.no_grad():
        attn = clf.get_embedding(torch.from_numpy(x))[2].view(8, len(lines), 25, 25)
    mean = attn.mean(0).cpu().numpy()
    for i, k in enumerate(sizes):
        blk = z["attn_mean"][z["offsets"][i]:z["offsets"][i + 1]].reshape(k, k)
        assert np.array_equal(blk, mean[i, :k, :k]), i
        hb = z["attn_heads"][8 * z["offsets"][i]:8 * z["offsets"][i + 1]].reshape(8, k, k)
        assert np.array_equal(hb, attn[:, i, :k, :k].cpu().numpy()), i
    # chunks of 7 rows are padded to their own longest row: a narrow chunk (<= 8 columns) goes through the short path
    small = PR.attention_maps(clf, [[int(v) for v in r] for r in lines], batch_size=7)
    assert small["sizes"].tolist() == sizes and small["attn_mean"].shape == z["attn_mean"].shape
    assert np.abs(small["attn_mean"] - z["attn_mean"]).max() > 1e-3                    # the chunk's width is part of the result
    # a 33-bin line is refused by its number before anything is scored
    write(inp, lines[:10] + [np.arange(1, 34)] + lines[10:])
    os.remove(out)
    with pytest.raises(ValueError, match=r"line 11 has 33 distinct bins"):
        PR.main(["attention", "-i", inp, "-o", out, "--config", cpath])
    assert not os.path.exists(out)
